"""Worlds as pixels, on the device: frames and segmentation masks of every scene, differentiable.

The reference draws through pygame (`Body.draw`, `physics/bodies.py:140-150`, `237-250`; the paint loop of `run_world`,
`world.py:279-280`) and records frames with `Recorder` (`utils.py:54-72`); its vision experiments
(`experiments/breakout/encoder.py`) consume those pixels.  Here ONE launch of `lcp_render_f64` (lcp_render.hip) turns geometry and
pose into `image [B,C,H,W]` float32 and `ids [B,H,W]` int32 for every scene, and ONE launch of `lcp_render_backward_f64` is its
backward, so a loss on pixels reaches the pose, the radii, the hull vertices and the colours - and, through
`ContactWorld.step(differentiable=True)`, everything upstream:

    cam = Camera(64, 64, origin=(440.0, 420.0), pixels_per_meter=0.5)
    img = world.render(cam, colors)                  # [B,3,64,64]; part of the roll-out's graph after differentiable steps
    ((img - target) ** 2).mean().backward()

Conventions (include/lcp_hip.h has the formulas): pixel (row i, column j) is sampled at the world point
`(x0 + (j + 1/2) / ppm, y0 + (i + 1/2) / ppm)`, x to the right and y downward; bodies are painted in list order, later over
earlier; `thickness == 0` is filled, `> 0` an outline; edges are a linear ramp of width `edge_width` (one pixel by default) in the
signed distance.  Not drawn: the circle's spoke, the hull's centre dot, the joints' markers.  No CPU fallback.
"""
from dataclasses import dataclass

import torch

from .. import _lib


@dataclass(frozen=True)
class Camera:
    """`height` x `width` pixels; `origin`: the world point of the image's top-left corner; `pixels_per_meter`: the reference's
    `Defaults.PIXELS_PER_METER`-style scale (pixel = (pos - origin) * pixels_per_meter)."""
    height: int
    width: int
    origin: tuple = (0.0, 0.0)
    pixels_per_meter: float = 1.0

    def __post_init__(self):
        if self.height < 1 or self.width < 1 or not self.pixels_per_meter > 0:
            raise ValueError("a camera needs at least one pixel each way and a positive scale")


def _geometry(geom, p):
    """The values of (radius, verts_local, p), after the checks every entry makes of the `GeometryBatch` `geom` and the pose."""
    _lib.require_gpu_tensor(geom.kind, "geom.kind", torch.int32)
    _lib.require_gpu_tensor(geom.nverts, "geom.nverts", torch.int32)
    r = _lib.require_gpu_tensor(geom.radius.detach(), "geom.radius", torch.float64)
    v = _lib.require_gpu_tensor(geom.verts_local.detach(), "geom.verts_local", torch.float64)
    pd = _lib.require_gpu_tensor(p.detach(), "p", torch.float64)
    if pd.shape != (geom.B, geom.nb, 3):
        raise ValueError("p must be [B,nb,3] = %s (got %s)" % ((geom.B, geom.nb, 3), tuple(pd.shape)))
    return r, v, pd


class _Launch:
    """The arguments both entries share, resolved once: sizes, camera, device pointers of the constant inputs."""

    def __init__(self, geom, cam, C, background, thickness, edge_width):
        self.sizes = (geom.B, geom.nb, geom.nvcap, geom.verts_max(), int(cam.height), int(cam.width), int(C))
        w = 1.0 / cam.pixels_per_meter if edge_width is None else float(edge_width)
        if not w > 0:
            raise ValueError("edge_width must be positive")
        self.cam = (float(cam.origin[0]), float(cam.origin[1]), float(cam.pixels_per_meter), w)
        self.kind, self.nverts = geom.kind, geom.nverts
        self.background = _lib.require_gpu_tensor(background, "background", torch.float32)
        if self.background.shape != (C,):
            raise ValueError("background must be [C] = [%d]" % C)
        self.thickness = None if thickness is None else _lib.require_gpu_tensor(thickness, "thickness", torch.float64)
        if self.thickness is not None and self.thickness.shape != (geom.B, geom.nb):
            raise ValueError("thickness must be [B,nb]")

    def inputs(self, radius, verts_local, p, colors):
        P = _lib.ptr
        return (*self.sizes, P(self.kind), P(radius), P(verts_local), P(self.nverts), P(p), P(colors), P(self.background),
                P(self.thickness), *self.cam)


class RenderFunction(torch.autograd.Function):
    """(p, radius, verts_local, colors [B,nb,C]) -> image [B,C,H,W]: one launch each way.  The backward asks the kernel only for
    the gradients autograd needs (NULL for the rest) and recomputes from the saved INPUTS; the image is not kept."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, colors, launch, out, ids_out):
        lib = _lib.load()
        dev = p.device
        B, _, _, _, H, W, C = launch.sizes
        image = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if out is None else out
        with _lib.on_device(dev):
            rc = lib.lcp_render_f64(*launch.inputs(radius, verts_local, p, colors), _lib.ptr(image), _lib.ptr(ids_out),
                                    _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_render_f64")
        ctx.launch = launch
        ctx.save_for_backward(p, radius, verts_local, colors)
        if out is not None:
            ctx.mark_dirty(out)
        return image

    @staticmethod
    def backward(ctx, g_image):
        p, radius, verts_local, colors = ctx.saved_tensors
        lib = _lib.load()
        dev = p.device
        g_image = g_image.to(torch.float32).contiguous()
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need else None
                for t, need in zip((p, radius, verts_local, colors), ctx.needs_input_grad[:4])]
        if all(o is None for o in outs):
            return (None,) * 7
        with _lib.on_device(dev):
            rc = lib.lcp_render_backward_f64(*ctx.launch.inputs(radius, verts_local, p, colors), _lib.ptr(g_image),
                                             *[_lib.ptr(o) for o in outs], _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_render_backward_f64")
        return (*outs, None, None, None)


def _colors(colors, geom):
    if colors.dim() == 2:
        colors = colors.unsqueeze(0).expand(geom.B, -1, -1)           # (autograd sums the scenes' gradients back)
    if colors.dim() != 3 or colors.shape[:2] != (geom.B, geom.nb) or not 1 <= colors.shape[2] <= 4:
        raise ValueError("colors must be [nb,C] or [B,nb,C] with 1 <= C <= 4 (got %s)" % (tuple(colors.shape),))
    if not colors.is_cuda:
        raise RuntimeError("colors must live on a GPU (got %s); the HIP path has no CPU fallback" % colors.device)
    return colors.to(torch.float32).contiguous()


def render(geom, p, cam, colors, background=None, thickness=None, edge_width=None, out=None, ids_out=None):
    """The frames of B scenes: `image [B,C,H,W]` float32, differentiable with respect to `p` [B,nb,3] f64, `geom.radius`,
    `geom.verts_local` and `colors` ([nb,C] shared by the scenes, or [B,nb,C]; float32, C in 1..4).
    `background` [C] float32 on the device (None: zeros); `thickness` [B,nb] f64 on the device (None: every body filled);
    `edge_width`: the ramp's width in world units (None: one pixel); `out` / `ids_out`: preallocated image [B,C,H,W] float32 and
    mask [B,H,W] int32 to write into.  With `out`, `background` and contiguous float32 [B,nb,C] `colors` given, a call is the one
    launch and nothing else (it can be captured in a `torch.cuda.graph`)."""
    pd = _geometry(geom, p)[2]
    colors = _colors(colors, geom)
    C = colors.shape[2]
    if background is None:
        background = torch.zeros(C, dtype=torch.float32, device=pd.device)
    if out is not None:
        _lib.require_gpu_tensor(out, "out", torch.float32)
        if out.shape != (geom.B, C, cam.height, cam.width):
            raise ValueError("out must be [B,C,H,W]")
    if ids_out is not None:
        _lib.require_gpu_tensor(ids_out, "ids_out", torch.int32)
        if ids_out.shape != (geom.B, cam.height, cam.width):
            raise ValueError("ids_out must be [B,H,W]")
    launch = _Launch(geom, cam, C, background, thickness, edge_width)
    return RenderFunction.apply(p, geom.radius, geom.verts_local, colors, launch, out, ids_out)


def render_ids(geom, p, cam, out=None):
    """The segmentation masks `ids [B,H,W]` int32: the index of the topmost body whose (filled) silhouette covers the pixel's
    centre, -1 where there is none.  No image is computed."""
    lib = _lib.load()
    radius, verts_local, pd = _geometry(geom, p)
    dev = pd.device
    if out is None:
        out = torch.empty(geom.B, cam.height, cam.width, dtype=torch.int32, device=dev)
    _lib.require_gpu_tensor(out, "out", torch.int32)
    if out.shape != (geom.B, cam.height, cam.width):
        raise ValueError("out must be [B,H,W]")
    dummy = torch.zeros(geom.B * geom.nb + 1, dtype=torch.float32, device=dev)          # colours / background of an image nobody asks for
    launch = _Launch(geom, cam, 1, dummy[:1], None, None)
    with _lib.on_device(dev):
        rc = lib.lcp_render_f64(*launch.inputs(radius, verts_local, pd, dummy[1:]), None, _lib.ptr(out), _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_render_f64")
    return out


class FrameRecorder:
    """The batched `Recorder` (utils.py:54-72): `record()` renders the world's current state and appends it as uint8 to a
    preallocated `[capacity,B,C,H,W]` device tensor - device operations only, no host synchronisation; `frames()` is the filled
    part, `save(dir, scene)` writes one scene's frames as PNG files (`frame_00000.png`, ...) through PIL."""

    def __init__(self, world, cam, colors, capacity, **render_kw):
        self.world, self.cam, self.kw = world, cam, render_kw
        self.colors = _colors(colors.detach(), world.geom)
        dev = world.p.device
        B, C = world.geom.B, self.colors.shape[2]
        self.kw.setdefault("background", torch.zeros(C, dtype=torch.float32, device=dev))
        self.capacity, self.count = int(capacity), 0
        self.buf = torch.zeros(self.capacity, B, C, cam.height, cam.width, dtype=torch.uint8, device=dev)
        self._image = torch.empty(B, C, cam.height, cam.width, dtype=torch.float32, device=dev)

    def record(self):
        if self.count >= self.capacity:
            raise RuntimeError("the recorder holds %d frames and is full" % self.capacity)
        with torch.no_grad():
            img = render(self.world.geom, self.world.p, self.cam, self.colors, out=self._image, **self.kw)
            self.buf[self.count].copy_(torch.round(img.clamp(0.0, 1.0) * 255.0))
        self.count += 1

    def frames(self):
        return self.buf[:self.count]

    def save(self, directory, scene=0):
        """Write scene `scene`'s frames to `directory` (created when missing); returns the paths.  C = 1: greyscale, 3: RGB,
        4: RGBA; C = 2 has no PNG mode and raises ValueError."""
        import os
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("FrameRecorder.save writes PNG files through PIL (the `pillow` package), which is not installed; "
                               "`frames()` gives the recorded tensor without it") from e
        C = self.buf.shape[2]
        if C == 2:
            raise ValueError("no PNG mode for %d channels" % C)
        os.makedirs(directory, exist_ok=True)
        host = self.frames()[:, scene].permute(0, 2, 3, 1).contiguous().cpu().numpy()
        paths = []
        for k in range(host.shape[0]):
            path = os.path.join(directory, "frame_%05d.png" % k)
            Image.fromarray(host[k, :, :, 0] if C == 1 else host[k]).save(path)      # (mode from the shape: L / RGB / RGBA)
            paths.append(path)
        return paths
