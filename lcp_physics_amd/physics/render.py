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
signed distance.  No CPU fallback.

The rest of the paint loop - the circle's spoke, the rect's diagonals, the hull's centre dot (`bodies.py:143-147, 244-247, 291-296`)
and the joints' markers (`constraints.py:51-206`, painted after the bodies, `world.py:281-282`) - comes with `marks=` and `joints=`:
ONE launch of `lcp_render_marks_f64` (lcp_render_marks.hip), and `lcp_render_marks_backward_f64` for its backward.  With a spoke a
circle's image depends on its angle, and the markers carry the joints' angles `jrot1` and anchor radii `jr1`, so a pixel loss reaches
a ball's spin and the joints' state:

    img = world.render(cam, colors, marks=marks_of(shapes), joints=True, marks_over=True)
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


NONE, SPOKE, CENTRE, DIAGONALS = 0, 1, 2, 3          # the codes of `marks`


def marks_of(shapes):
    """The reference's mark for every body of the list given to `GeometryBatch.from_shapes` / `BodyBatch.from_list`: a circle gets
    its spoke (bodies.py:144-147), a rect its diagonals (:295-296), any other hull its centre dot (:245-247).  [nb] int32 (CPU)."""
    code = {"circle": SPOKE, "rect": DIAGONALS, "hull": CENTRE}
    return torch.tensor([code[s[0]] for s in shapes], dtype=torch.int32)


class _Marks:
    """What the two entries with marks and markers take on top of `_Launch`: the constant inputs, resolved once."""

    def __init__(self, geom, cam, marks, joints, marks_over, mark_width, dot_radius, joint_width, joint_radius):
        B, nb, ppm = geom.B, geom.nb, float(cam.pixels_per_meter)
        if marks is not None:
            if marks.dim() == 1:
                marks = marks.unsqueeze(0).expand(B, -1)
            if marks.shape != (B, nb):
                raise ValueError("marks must be [nb] or [B,nb] (got %s)" % (tuple(marks.shape),))
            marks = _lib.require_gpu_tensor(marks.contiguous(), "marks", torch.int32)
        self.marks, self.joints = marks, joints
        self.nj = 0
        if joints is not None:
            self.nj = int(joints.jtype.shape[1])
            for name in ("jtype", "jb1", "jb2"):
                t = _lib.require_gpu_tensor(getattr(joints, name), "joints." + name, torch.int32)
                if t.shape != (B, self.nj):
                    raise ValueError("joints.%s must be [B,nj]" % name)
            if self.nj > 64:
                raise ValueError("at most 64 joints are drawn (got %d)" % self.nj)
        # the reference's pixel sizes: lines 1, dots 2, the joints' lines 2 and ticks / rings 5 pixels
        px = lambda v, n: n / ppm if v is None else float(v)
        self.consts = (int(bool(marks_over)), px(mark_width, 1.0), px(dot_radius, 2.0), px(joint_width, 2.0), px(joint_radius, 5.0))
        if not (self.consts[1] > 0 and self.consts[3] > 0 and self.consts[2] >= 0 and self.consts[4] >= 0):
            raise ValueError("mark_width and joint_width must be positive, dot_radius and joint_radius not negative")

    def inputs(self, mark_colors, jr1, jrot1, joint_colors):
        P, js = _lib.ptr, self.joints
        if self.nj == 0:
            return (P(self.marks), P(mark_colors), 0, None, None, None, None, None, None, *self.consts)
        return (P(self.marks), P(mark_colors), self.nj, P(js.jtype), P(js.jb1), P(js.jb2), P(jr1), P(jrot1), P(joint_colors), *self.consts)


class RenderMarksFunction(torch.autograd.Function):
    """(p, radius, verts_local, colors, mark_colors, joint_colors, jrot1, jr1) -> image [B,C,H,W]: `RenderFunction` with the marks
    and the joints' markers.  One launch forward; backward one launch, and a second small one that adds the joints' pull on their
    bodies to the pose gradient.  The kernel is asked only for the gradients autograd needs; inputs are saved, not the image."""

    @staticmethod
    def forward(ctx, p, radius, verts_local, colors, mark_colors, joint_colors, jrot1, jr1, launch, mk, out, ids_out):
        lib = _lib.load()
        dev = p.device
        B, _, _, _, H, W, C = launch.sizes
        image = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if out is None else out
        with _lib.on_device(dev):
            rc = lib.lcp_render_marks_f64(*launch.inputs(radius, verts_local, p, colors), *mk.inputs(mark_colors, jr1, jrot1, joint_colors),
                                          _lib.ptr(image), _lib.ptr(ids_out), _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_render_marks_f64")
        ctx.launch, ctx.mk = launch, mk
        ctx.save_for_backward(p, radius, verts_local, colors, mark_colors, joint_colors, jrot1, jr1)
        if out is not None:
            ctx.mark_dirty(out)
        return image

    @staticmethod
    def backward(ctx, g_image):
        saved = ctx.saved_tensors
        p, radius, verts_local, colors, mark_colors, joint_colors, jrot1, jr1 = saved
        lib = _lib.load()
        dev = p.device
        mk = ctx.mk
        g_image = g_image.to(torch.float32).contiguous()
        # (an input that is not there - no marks, no joints - is None and asks for nothing)
        outs = [torch.empty(t.shape, dtype=t.dtype, device=dev) if need and t is not None else None
                for t, need in zip(saved, ctx.needs_input_grad[:8])]
        if mk.nj == 0:                                                # (empty tensors: nothing to write)
            outs[5:8] = [o if o is None else torch.zeros_like(o) for o in outs[5:8]]
        asked = [None if (o is None or o.numel() == 0) else o for o in outs]
        if all(o is None for o in asked):
            return (*outs, None, None, None, None)
        ws = None
        if asked[0] is not None and mk.nj > 0:
            ws = torch.empty(p.shape[0], mk.nj, 2, 3, dtype=torch.float64, device=dev)
        with _lib.on_device(dev):
            rc = lib.lcp_render_marks_backward_f64(*ctx.launch.inputs(radius, verts_local, p, colors),
                                                   *mk.inputs(mark_colors, jr1, jrot1, joint_colors), _lib.ptr(g_image),
                                                   *[_lib.ptr(o) for o in asked], _lib.ptr(ws), _lib.stream_ptr(dev))
        _lib.check(rc, "lcp_render_marks_backward_f64")
        return (*outs, None, None, None, None)


def _layer_colors(colors, B, n, C, default, what):
    """Colours of the marks / the joints' markers: [n,C] shared by the scenes or [B,n,C]; None: the reference's (C >= 3 only)."""
    if colors is None:
        if C < 3:
            raise ValueError("%s has no default for %d channel(s): the reference's is an RGB colour" % (what, C))
        return default(C).reshape(1, 1, C).expand(B, n, C).contiguous()
    if colors.dim() == 2:
        colors = colors.unsqueeze(0).expand(B, -1, -1)
    if colors.shape != (B, n, C):
        raise ValueError("%s must be [%d,%d] or [%d,%d,%d] (got %s)" % (what, n, C, B, n, C, tuple(colors.shape)))
    if not colors.is_cuda:
        raise RuntimeError("%s must live on a GPU (got %s); the HIP path has no CPU fallback" % (what, colors.device))
    return colors.to(torch.float32).contiguous()


def _colors(colors, geom):
    if colors.dim() == 2:
        colors = colors.unsqueeze(0).expand(geom.B, -1, -1)           # (autograd sums the scenes' gradients back)
    if colors.dim() != 3 or colors.shape[:2] != (geom.B, geom.nb) or not 1 <= colors.shape[2] <= 4:
        raise ValueError("colors must be [nb,C] or [B,nb,C] with 1 <= C <= 4 (got %s)" % (tuple(colors.shape),))
    if not colors.is_cuda:
        raise RuntimeError("colors must live on a GPU (got %s); the HIP path has no CPU fallback" % colors.device)
    return colors.to(torch.float32).contiguous()


def render(geom, p, cam, colors, background=None, thickness=None, edge_width=None, out=None, ids_out=None, marks=None,
           mark_colors=None, joints=None, jrot1=None, joint_colors=None, marks_over=False, mark_width=None, dot_radius=None,
           joint_width=None, joint_radius=None):
    """The frames of B scenes: `image [B,C,H,W]` float32, differentiable with respect to `p` [B,nb,3] f64, `geom.radius`,
    `geom.verts_local` and `colors` ([nb,C] shared by the scenes, or [B,nb,C]; float32, C in 1..4).
    `background` [C] float32 on the device (None: zeros); `thickness` [B,nb] f64 on the device (None: every body filled);
    `edge_width`: the ramp's width in world units (None: one pixel); `out` / `ids_out`: preallocated image [B,C,H,W] float32 and
    mask [B,H,W] int32 to write into.  With `out`, `background` and contiguous float32 [B,nb,C] `colors` given, a call is the one
    launch and nothing else (it can be captured in a `torch.cuda.graph`).

    `marks` ([nb] or [B,nb] int32 on the device: NONE / SPOKE / CENTRE / DIAGONALS, see `marks_of`) draws the bodies' marks in
    `mark_colors` ([nb,C] or [B,nb,C]; None: the reference's blue, C >= 3), `joints` (a `JointSet`) the joints' markers in
    `joint_colors` ([nj,C] or [B,nj,C]; None: the reference's green) at the angles `jrot1` [B,nj] f64 (None: `joints.jrot1`); the image
    is then differentiable with respect to the two colour tensors, `jrot1` and `joints.jr1` as well.  `marks_over=False` is the
    reference's order (spoke and diagonals under their body, centre dot over it), `True` paints every mark over its body - what shows on
    a filled body.  `mark_width`, `dot_radius`, `joint_width`, `joint_radius`: world lengths (None: 1, 2, 2 and 5 pixels).  With
    neither `marks` nor `joints` the call is today's `lcp_render_f64`; with `out`, `background` and contiguous inputs given a call
    with marks is one launch and nothing else, too."""
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
    if marks is None and joints is None:
        return RenderFunction.apply(p, geom.radius, geom.verts_local, colors, launch, out, ids_out)
    mk = _Marks(geom, cam, marks, joints, marks_over, mark_width, dot_radius, joint_width, joint_radius)
    dev = pd.device
    if marks is not None:
        blue = lambda C: torch.tensor([0.0, 0.0, 1.0, 1.0][:C], dtype=torch.float32, device=dev)
        mark_colors = _layer_colors(mark_colors, geom.B, geom.nb, C, blue, "mark_colors")
    else:
        mark_colors = None
    jr1 = None
    if joints is not None:
        green = lambda C: torch.tensor([0.0, 1.0, 0.0, 1.0][:C], dtype=torch.float32, device=dev)
        joint_colors = _layer_colors(joint_colors, geom.B, mk.nj, C, green, "joint_colors")
        jrot1, jr1 = (joints.jrot1 if jrot1 is None else jrot1).contiguous(), joints.jr1.contiguous()
        for name, t in (("jrot1", jrot1), ("joints.jr1", jr1)):
            _lib.require_gpu_tensor(t.detach(), name, torch.float64)
            if t.shape != (geom.B, mk.nj):
                raise ValueError("%s must be [B,nj]" % name)
    else:
        joint_colors = jrot1 = None
    return RenderMarksFunction.apply(p, geom.radius, geom.verts_local, colors, mark_colors, joint_colors, jrot1, jr1, launch, mk, out,
                                     ids_out)


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
    """The batched `Recorder` (utils.py:54-72; keywords of `render` pass through, `joints=True` stands for the world's `JointSet`
    at every `record()`): `record()` renders the world's current state and appends it as uint8 to a
    preallocated `[capacity,B,C,H,W]` device tensor - device operations only, no host synchronisation; `frames()` is the filled
    part, `save(dir, scene)` writes one scene's frames as PNG files (`frame_00000.png`, ...) through PIL."""

    def __init__(self, world, cam, colors, capacity, **render_kw):
        self.world, self.cam, self.kw = world, cam, render_kw          # (marks=, joints=True, ... pass through to `render`)
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
            kw = dict(self.kw)
            if kw.get("joints") is True:                              # the world's joints at their current angles
                kw["joints"] = self.world._joints_to_draw()
            elif kw.get("joints") is False:
                kw["joints"] = None
            img = render(self.world.geom, self.world.p, self.cam, self.colors, out=self._image, **kw)
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
