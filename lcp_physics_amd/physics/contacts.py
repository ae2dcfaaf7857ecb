"""Batched narrow-phase contact generation on the GPU.

Host-side mirror of the reference's contact pipeline for B independent scenes:
`World.find_contacts` (`physics/world.py:139-142`) + `DiffContactHandler.__call__`
(`physics/contacts.py:57-205`) + the move / penetration-check / dt-halving loop of `World.step_dt`
(`world.py:88-101`), all inside ONE launch of `lcp_move_find_contacts_f64` (include/lcp_hip.h).
The contact record has the reference's format `((normal, p1, p2, penetration), i1, i2)`
(`contacts.py:203-204`), stored structure-of-arrays and padded to `maxc` contacts per scene with a
per-scene `count`.  No CPU fallback.

Sizes: hulls of up to 8 vertices in scenes of up to 32 bodies run on `lcp_move_find_contacts_f64` /
`lcp_contact_frame_backward_f64` (lcp_contacts.hip); anything else, up to 64 vertices per hull (the capacity
`verts_local.shape[2]`, 8..64), 64 bodies and 1024 hull vertices per scene, on the `_nv_` entries (lcp_contacts_wide.hip).
`broadphase=True` (opt-in) runs the detection at all of these sizes on `lcp_move_find_contacts_bp_f64` (lcp_contacts_bp.hip): the pairs
are culled by bounding circle and bounding box before the narrow phase, the records are the same bit for bit.
"""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib

CIRCLE, HULL = 0, 1
NV = 8                   # default vertex capacity of a hull (lcp_contacts.hip)
NV_MAX = 64              # largest capacity / hull (lcp_contacts_wide.hip)
NB_SMALL = 32            # bodies per scene of the lcp_contacts.hip entries
EPSILON = 0.1            # physics/utils.py:16  (contact detection margin)
TOL = 1e-6               # physics/utils.py:17  (allowed penetration)


@dataclass
class GeometryBatch:
    """Collision geometry of the bodies of B scenes (constant over a simulation).

    kind [B,nb] int32 (0 circle, 1 hull), radius [B,nb] f64, verts_local [B,nb,cap,2] f64 (body frame, the
    order of the reference's `Hull.verts`; cap = 8 by default, up to 64), nverts [B,nb] int32, no_contact [B,nb,nb]
    uint8 or None (the pairs `World` excludes through `add_no_contact`, bodies.py:117-118).
    scene_verts_max: the largest sum of hull vertices over one scene (a host int: it sizes the LDS of the wide kernels);
    `from_shapes` sets it, otherwise it is computed on first use (one synchronisation) and cached - rebuild the batch
    rather than editing `nverts` in place.

    `radius` and `verts_local` may require grad (or carry a graph: one learnable shape expanded over the B scenes, say):
    `ContactWorld.step(differentiable=True)` then back-propagates to them through the contact frame
    (`contact_frame_backward_shape`), as the reference's autograd does to `Circle.rad` / `Hull.verts`.  The kernels read
    their values only.  A batch built by hand (or by `from_shapes`) takes vertices that are convex, in the reference's order and
    centred on the centroid, and leaves `Mdiag` to the caller; `physics.bodies.BodyBatch.from_list` does what the reference's
    `Hull.__init__` does instead - validation, centroid, recentred vertices, position, inertia, mass matrix, gravity from the raw
    shape and the mass in one launch (`lcp_body_properties_f64`), differentiable - and hands out a `GeometryBatch` whose `radius` and
    `verts_local` carry that graph."""
    kind: torch.Tensor
    radius: torch.Tensor
    verts_local: torch.Tensor
    nverts: torch.Tensor
    no_contact: torch.Tensor = None
    scene_verts_max: int = None

    @property
    def B(self):
        return self.kind.shape[0]

    @property
    def nb(self):
        return self.kind.shape[1]

    @property
    def nvcap(self):
        """Vertex capacity of a hull in `verts_local`."""
        return self.verts_local.shape[2]

    def verts_max(self):
        """`scene_verts_max`, computed once (one device read) when it was not given."""
        if self.scene_verts_max is None:
            n = torch.where(self.kind != CIRCLE, self.nverts.clamp(0, self.nvcap), torch.zeros_like(self.nverts))
            self.scene_verts_max = int(n.sum(dim=1).max()) if n.numel() else 0
        return self.scene_verts_max

    @property
    def wide(self):
        """True when the sizes need the lcp_contacts_wide.hip entries (capacity other than 8 or more than 32 bodies)."""
        return self.nvcap != NV or self.nb > NB_SMALL

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device).contiguous()     # (differentiable: a graph on radius / verts_local survives)
        return GeometryBatch(mv(self.kind), mv(self.radius), mv(self.verts_local), mv(self.nverts), mv(self.no_contact),
                             self.scene_verts_max)

    @staticmethod
    def from_shapes(shapes, B=1, max_verts=NV):
        """`shapes`: per body ('circle', rad) or ('rect', (w, h)) or ('hull', verts[nv,2]); replicated B times.
        A radius or a vertex array given as a tensor that requires grad stays connected: `radius` / `verts_local` of the
        batch are then functions of it (autograd sums over the B replicas).
        `max_verts`: the vertex capacity of `verts_local` (8 .. 64; a larger hull raises ValueError); None: the largest hull's
        vertex count, at least 8."""
        nb = len(shapes)
        vlists = []
        live = lambda a: isinstance(a, torch.Tensor) and a.requires_grad
        for k, a in shapes:
            if k == "circle":
                vlists.append(None)
            elif live(a) and k != "rect":
                vlists.append(a.detach().to(torch.float64).tolist())
            elif k == "rect":                        # bodies.py:261-264: [half, half * (-1, 1), -half, -half * (-1, 1)]
                hw, hh = float(a[0]) / 2, float(a[1]) / 2
                vlists.append([[hw, hh], [-hw, hh], [-hw, -hh], [hw, -hh]])
            else:
                vlists.append(np.asarray(a, dtype=np.float64).tolist())
        largest = max([len(v) for v in vlists if v is not None], default=0)
        cap = max(NV, largest) if max_verts is None else int(max_verts)
        if not NV <= cap <= NV_MAX:
            raise ValueError("the vertex capacity must lie in [%d, %d] (got %d)" % (NV, NV_MAX, cap))
        kind = torch.zeros(nb, dtype=torch.int32)
        radius = torch.zeros(nb, dtype=torch.float64)
        verts = torch.zeros(nb, cap, 2, dtype=torch.float64)
        nverts = torch.zeros(nb, dtype=torch.int32)
        for i, ((k, a), vs) in enumerate(zip(shapes, vlists)):
            if k == "circle":
                kind[i], radius[i] = CIRCLE, float(a.detach() if live(a) else a)
            else:
                if len(vs) > cap:
                    raise ValueError("hulls are limited to %d vertices" % cap)
                kind[i], nverts[i] = HULL, len(vs)
                verts[i, :len(vs)] = torch.tensor(vs, dtype=torch.float64)
        for i, (k, a) in enumerate(shapes):                  # learnable shapes: the same values, with their graph
            if live(a) and k == "circle":
                radius = radius.index_put((torch.tensor(i),), a.to(torch.float64).reshape(()))
            elif live(a) and k != "rect":
                verts = torch.cat([verts[:i], torch.cat([a.to(torch.float64), verts[i, a.shape[0]:]]).unsqueeze(0), verts[i + 1:]])
        rep = lambda t: t.unsqueeze(0).repeat(B, *([1] * t.dim())).contiguous()
        return GeometryBatch(rep(kind), rep(radius), rep(verts), rep(nverts), None, int(nverts.sum()))


class ContactBuffers:
    """Device buffers the contact kernel fills (allocated once and re-used every step by `ContactWorld.step`; one fresh set per
    differentiable step, which keeps the previous set as that step's contact snapshot).  ONE zero-filled allocation, carved into
    the typed arrays: a single memset launch instead of twelve."""

    _LAYOUTS = {}                                                    # (B, nb, maxc) -> total bytes, [(name, dtype, shape, offset, bytes)]

    @classmethod
    def _layout(cls, B, nb, maxc):
        key = (B, nb, maxc)
        lay = cls._LAYOUTS.get(key)
        if lay is None:
            spec = (("p_out", torch.float64, (B, nb, 3)), ("c_pen", torch.float64, (B, maxc)), ("max_pen", torch.float64, (B,)),
                    ("dt_used", torch.float64, (B,)), ("c_n", torch.float32, (B, maxc, 2)), ("c_p1", torch.float32, (B, maxc, 2)),
                    ("c_p2", torch.float32, (B, maxc, 2)), ("c_i1", torch.int32, (B, maxc)), ("c_i2", torch.int32, (B, maxc)),
                    ("count", torch.int32, (B,)), ("trials", torch.int32, (B,)))
            off, items = 0, []
            for name, dt, sh in spec:
                n = int(np.prod(sh)) * (8 if dt == torch.float64 else 4)
                items.append((name, dt, sh, off, n))
                off += (n + 15) // 16 * 16
            lay = cls._LAYOUTS[key] = (off, items)
        return lay

    def __init__(self, B, nb, maxc, device):
        self.maxc = maxc
        total, items = self._layout(B, nb, maxc)
        self._carve(torch.zeros(total, dtype=torch.uint8, device=device), items)

    def _carve(self, backing, items):
        self._backing, self._dims = backing, None
        for name, dt, sh, off, n in items:
            setattr(self, name, backing[off:off + n].view(dt).view(sh))

    def clone(self):
        """A copy in storage of its own (one device copy): what a world keeps when the original became part of an autograd graph."""
        B, nb = self.p_out.shape[0], self.p_out.shape[1]
        new = ContactBuffers.__new__(ContactBuffers)
        new.maxc = self.maxc
        new._carve(self._backing.clone(), self._layout(B, nb, self.maxc)[1])
        if self.p_out.data_ptr() != self._backing.data_ptr():          # (ContactWorld.step swaps p_out with its pose buffer)
            new.p_out = self.p_out.clone()
        return new


def _check_geometry(geom, p, name):
    """The geometry tensors every entry reads and the pose they are evaluated at (`name`, [B,nb,3] float64).  Returns B, nb."""
    B, nb, cap = geom.B, geom.nb, geom.nvcap
    _lib.require_gpu_tensor(geom.kind, "kind", torch.int32)
    _lib.require_gpu_tensor(geom.nverts, "nverts", torch.int32)
    _lib.require_gpu_tensor(geom.radius, "radius", torch.float64)
    _lib.require_gpu_tensor(geom.verts_local, "verts_local", torch.float64)
    _lib.require_gpu_tensor(p, name, torch.float64)
    if tuple(p.shape) != (B, nb, 3) or tuple(geom.verts_local.shape) != (B, nb, cap, 2) or not NV <= cap <= NV_MAX:
        raise RuntimeError("%s must be [B,nb,3] and verts_local [B,nb,cap,2] with %d <= cap <= %d" % (name, NV, NV_MAX))
    if geom.no_contact is not None:
        _lib.require_gpu_tensor(geom.no_contact, "no_contact", torch.uint8)
    return B, nb


def _entry(geom, stem, sizes, dt_scene=None, broadphase=False, candidates=None):
    """Which C entry serves a call: its symbol, its leading size arguments (`sizes` = B, nb, maxc, then the vertex capacity and the
    scene's vertex total where the entry takes them) and what follows the common arguments, the stream apart.  `stem`:
    "lcp_move_find_contacts" or "lcp_contact_frame_backward" (which has neither a per-scene dt nor a broadphase).  The kernels behind
    each symbol: `route_contacts` in lcp_api.cpp.  `geom.verts_max()` may synchronise once, so only the routes whose kernels need the
    vertex total evaluate it (`ContactWorld` captures its steps into HIP graphs)."""
    if broadphase:                                      # (the real vertex total, also for a batch that is not `wide`)
        return stem + "_bp_f64", sizes + (geom.nvcap, geom.verts_max()), (_lib.ptr(dt_scene), _lib.ptr(candidates))
    if dt_scene is not None:
        return stem + "_dts_f64", sizes + (geom.nvcap, geom.verts_max() if geom.wide else 0), (_lib.ptr(dt_scene),)
    if geom.wide:
        return stem + "_nv_f64", sizes + (geom.nvcap, geom.verts_max()), ()
    return stem + "_f64", sizes, ()


def move_and_find_contacts(geom, p_start, v, dt, maxc=16, eps=EPSILON, tol=TOL, strict=True, dt_floor=None,
                           max_trials=64, t=None, out=None, dt_scene=None, broadphase=False, candidates=None):
    """`p <- p_start + v dt`, contacts at the new pose, dt halving while a contact penetrates by more than `tol`
    (`world.py:88-101`) for every scene.  `v=None` detects at `p_start` (the `find_contacts()` of
    `World.__init__`, `world.py:65-66`).  Returns the `ContactBuffers` (p_out = accepted pose).
    `dt_scene` [B] float64: every scene's loop starts from its own dt (`lcp_move_find_contacts_dts_f64`: the sub-steps of
    `World.step(fixed_dt=True)`, `world.py:72-80`); a scene with dt_scene <= 0 stays at `p_start` with dt_used = 0.  `dt` then only
    sets the default `dt_floor`.
    `broadphase=True`: the launch is `lcp_move_find_contacts_bp_f64` (lcp_contacts_bp.hip) at every size - each trial pose culls the
    body pairs by bounding circle and bounding box (the role of the ODE space of `World.find_contacts`, `world.py:139-142`, over the
    padded spheres of `bodies.py:_create_geom`) and only the survivors reach the narrow phase; the outputs are the same bit for bit.
    `candidates`: an optional [B] int32 device tensor that receives the number of surviving pairs at the accepted pose."""
    lib = _lib.load()
    B, nb = _check_geometry(geom, p_start, "p_start")
    if v is not None:
        _lib.require_gpu_tensor(v, "v", torch.float32)
    if t is not None:
        _lib.require_gpu_tensor(t, "t", torch.float64)
    dev = p_start.device
    if out is None:
        out = ContactBuffers(B, nb, maxc, dev)
    if dt_scene is not None:
        _lib.require_gpu_tensor(dt_scene, "dt_scene", torch.float64)
        if tuple(dt_scene.shape) != (B,):
            raise RuntimeError("dt_scene must be [B]")
    if candidates is not None:
        if not broadphase:
            raise ValueError("candidates belongs to broadphase=True")
        _lib.require_gpu_tensor(candidates, "candidates", torch.int32)
        if tuple(candidates.shape) != (B,):
            raise RuntimeError("candidates must be [B]")
    P = _lib.ptr
    name, sizes, tail = _entry(geom, "lcp_move_find_contacts", (B, nb, out.maxc), dt_scene, broadphase, candidates)
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(*sizes, P(geom.kind), P(geom.radius), P(geom.verts_local), P(geom.nverts), P(geom.no_contact),
                                P(p_start), P(v), float(dt), float(dt / 4 if dt_floor is None else dt_floor), int(bool(strict)),
                                int(max_trials), float(eps), float(tol), P(out.p_out), P(out.c_n), P(out.c_p1), P(out.c_p2),
                                P(out.c_pen), P(out.c_i1), P(out.c_i2), P(out.count), P(out.max_pen), P(out.dt_used), P(t),
                                P(out.trials), *tail, _lib.stream_ptr(dev))
    _lib.check(rc, name)
    return out


def find_contacts(geom, p, maxc=16, eps=EPSILON, out=None, broadphase=False, candidates=None):
    """`World.find_contacts` (`world.py:139-142`) for every scene at pose `p` [B,nb,3] (float64); `broadphase`, `candidates`: see
    `move_and_find_contacts`."""
    return move_and_find_contacts(geom, p, None, 0.0, maxc=maxc, eps=eps, out=out, max_trials=1, broadphase=broadphase,
                                  candidates=candidates)


def _check_cotangents(g_n, g_p1, g_p2):
    for name, t in (("g_n", g_n), ("g_p1", g_p1), ("g_p2", g_p2)):
        _lib.require_gpu_tensor(t, name, torch.float32)


def contact_frame_backward(geom, p, cb, g_n, g_p1, g_p2, eps=EPSILON):
    """d(loss)/d(pose) through the contact frame (`lcp_contact_frame_backward_f64`): the chain rule of the reference's
    differentiable contact handler (`contacts.py:57-352`) for the contacts in `cb` detected at pose `p` [B,nb,3] float64 with
    margin `eps` - every record type (circle / circle, circle / hull, hull / hull).  `cb`: the records (`ContactBuffers` or
    a snapshot: c_n, c_i1, c_i2, count)."""
    lib = _lib.load()
    B, nb = _check_geometry(geom, p, "p")
    _check_cotangents(g_n, g_p1, g_p2)
    dev = p.device
    dp = torch.empty(B, nb, 3, dtype=torch.float64, device=dev)
    P = _lib.ptr
    name, sizes, _ = _entry(geom, "lcp_contact_frame_backward", (B, nb, cb.c_n.shape[1]))
    pairs = (P(cb.c_i1), P(cb.c_i2)) if geom.wide else ()               # (the _nv_ entry reads the pairs from the records)
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(*sizes, P(geom.kind), P(geom.radius), P(geom.verts_local), P(geom.nverts), P(geom.no_contact), P(p),
                                float(eps), P(cb.count), *pairs, P(g_n), P(g_p1), P(g_p2), P(dp), _lib.stream_ptr(dev))
    _lib.check(rc, name)
    return dp


def contact_frame_backward_shape(geom, p, cb, g_n, g_p1, g_p2, eps=EPSILON, want_radius=True, want_verts=True):
    """d(loss)/d(radius) [B,nb] and d(loss)/d(verts_local) [B,nb,cap,2] through the contact frame
    (`lcp_contact_frame_backward_shape_f64`, lcp_contacts_shape.hip): what the reference's autograd gives `Circle.rad` and
    `Hull.verts` (`contacts.py:57-352` on `bodies.py:121, 168-171, 211-214`) for the contacts in `cb` detected at pose `p` with margin
    `eps`, along the branches the detection took.  One kernel for every geometry layout (capacity 8 .. 64, up to 64 bodies).
    Circles get zero vertex gradient, hulls zero radius gradient, vertex slots beyond `nverts` zero.  An output that is not
    wanted is None."""
    lib = _lib.load()
    B, nb = _check_geometry(geom, p, "p")
    _check_cotangents(g_n, g_p1, g_p2)
    dev = p.device
    d_rad = torch.empty(B, nb, dtype=torch.float64, device=dev) if want_radius else None
    d_verts = torch.empty(B, nb, geom.nvcap, 2, dtype=torch.float64, device=dev) if want_verts else None
    P = _lib.ptr
    with torch.cuda.device(dev):
        rc = lib.lcp_contact_frame_backward_shape_f64(B, nb, cb.c_n.shape[1], geom.nvcap, geom.verts_max(), P(geom.kind), P(geom.radius),
                                                      P(geom.verts_local), P(geom.nverts), P(p), float(eps), P(cb.count), P(cb.c_i1),
                                                      P(cb.c_i2), P(g_n), P(g_p1), P(g_p2), P(d_rad), P(d_verts), _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_contact_frame_backward_shape_f64")
    return d_rad, d_verts


class _FrameSnapshot:
    __slots__ = ("c_n", "c_p1", "c_p2", "c_i1", "c_i2", "count")


class ContactFrameFunction(torch.autograd.Function):
    """The contact list as a differentiable function of the poses: forward hands out the records the detection kernel
    found at `p` (their values are constants of the launch), backward is `lcp_contact_frame_backward_f64`.

        c_n, c_p1, c_p2 = ContactFrameFunction.apply(p, geom, frame)        # frame: a snapshot of the ContactBuffers

    With the optional trailing inputs `radius`, `verts_local` (pass `geom.radius` / `geom.verts_local` where they require grad, None
    otherwise) the records are functions of the shape too: backward then also runs `lcp_contact_frame_backward_shape_f64`.  Without
    them - or when neither needs a gradient - the backward is the pose kernel's launch alone."""

    @staticmethod
    def forward(ctx, p, geom, frame, eps=EPSILON, radius=None, verts_local=None):
        # The kernels write contact buffers through raw pointers (autograd's version counters never see it), so the records this node
        # hands out and keeps for its backward must belong to nobody else: a `snapshot_frame()`, or the ContactBuffers a
        # differentiable step RETIRED (`ContactWorld.step_autograd` marks them `retired`: the world detects into a fresh set from
        # then on) are used as they are; a LIVE buffer set (e.g. `world.contacts`) is copied first.
        if isinstance(frame, ContactBuffers) and not getattr(frame, "retired", False):
            frame = snapshot_frame(frame)
        ctx.geom, ctx.frame, ctx.eps = geom, frame, eps
        ctx.save_for_backward(p)
        return frame.c_n.detach(), frame.c_p1.detach(), frame.c_p2.detach()

    @staticmethod
    def backward(ctx, g_n, g_p1, g_p2):
        (p,) = ctx.saved_tensors
        z = lambda g, like: torch.zeros_like(like) if g is None else g.contiguous()
        fr = ctx.frame
        g_n, g_p1, g_p2 = z(g_n, fr.c_n), z(g_p1, fr.c_p1), z(g_p2, fr.c_p2)
        dp = contact_frame_backward(ctx.geom, p, fr, g_n, g_p1, g_p2, eps=ctx.eps) if ctx.needs_input_grad[0] else None
        d_rad = d_verts = None
        need = tuple(ctx.needs_input_grad) + (False, False)             # (as many entries as `apply` was given inputs)
        want_r, want_v = need[4], need[5]
        if want_r or want_v:
            d_rad, d_verts = contact_frame_backward_shape(ctx.geom, p, fr, g_n, g_p1, g_p2, eps=ctx.eps, want_radius=want_r,
                                                          want_verts=want_v)
        return (dp, None, None, None, d_rad, d_verts)[:len(ctx.needs_input_grad)]


def snapshot_frame(cb):
    """Copies of the contact records in `cb` (the buffers are re-used by the next detection launch)."""
    fr = _FrameSnapshot()
    fr.c_n, fr.c_p1, fr.c_p2 = cb.c_n.clone(), cb.c_p1.clone(), cb.c_p2.clone()
    fr.c_i1, fr.c_i2, fr.count = cb.c_i1.clone(), cb.c_i2.clone(), cb.count.clone()
    return fr
