"""Bodies on the device: what the reference's constructors compute from shape and mass.

`Circle`, `Rect` and `Hull` of the reference (`physics/bodies.py:15-290`) take a RAW description - a radius, the dims of a box, or
vertices relative to a reference point - and derive from it, inside autograd: the centroid (`bodies.py:216-226`), the vertices
recentred on it (`:171`), the position `ref_point + centroid` (`:173`), the angular inertia (`:125-126`, `:179-189`), the mass
matrix (`:44-47`) and, with `Gravity` attached, the force `(0, 0, m g)` (`forces.py:64-67`).  Here that is ONE launch of
`lcp_body_properties_f64` for every body of every scene (lcp_bodies.hip), its chain rule ONE launch of
`lcp_body_properties_backward_f64`:

    bodies = BodyBatch.from_list([("rect", [500, 500], [900, 10]),
                                  ("circle", [380, 468], rad, {"restitution": 0.3}),            # `rad`: a tensor that requires grad
                                  ("hull", [470, 474.5], verts, {"mass": mass})], B=96, g=100.0)
    world = bodies.world(Je=Je, dt=1 / 30, maxc=8)
    ...                                                                                          # step(differentiable=True), loss
    loss.backward()        # rad.grad, verts.grad, mass.grad: contact frame + mass matrix + initial position + gravity

No CPU fallback: the launches need a GPU; building the raw inputs (`BodyBatch.raw_inputs`) does not.
"""
from dataclasses import dataclass

import torch

from .. import _lib
from .contacts import CIRCLE, HULL, NV, NV_MAX, GeometryBatch

RESTITUTION = 0.5        # physics/utils.py (Defaults.RESTITUTION)
FRIC_COEFF = 0.9         # physics/utils.py (Defaults.FRIC_COEFF)
STATUS_NAMES = ((_lib.BODY_ST_COUNT, "fewer than 3 vertices or more than the capacity"),
                (_lib.BODY_ST_ORIENTATION, "vertices not in the reference's order (bodies.py:228-235)"),
                (_lib.BODY_ST_NONCONVEX, "not convex"),
                (_lib.BODY_ST_DEGENERATE, "no area, or a non-finite vertex, radius or mass"))


def _raw(t, name, dtype):
    t = t.detach()
    _lib.require_gpu_tensor(t, name, dtype)
    return t


def body_properties(kind, radius, verts_raw, nverts, mass, g=0.0, want=("centroid", "verts_local", "inertia", "Mdiag", "f_gravity",
                                                                       "status")):
    """`lcp_body_properties_f64` on device tensors: kind [B,nb] i32, radius [B,nb] f64, verts_raw [B,nb,cap,2] f64 (relative to the
    reference point, the reference's vertex order), nverts [B,nb] i32, mass [B,nb] f64 -> dict of the outputs named in `want`:
    centroid [B,nb,2] f64, verts_local [B,nb,cap,2] f64, inertia [B,nb] f64, Mdiag [B,nb,3] f32, f_gravity [B,nb,3] f32,
    status [B,nb] i32 (`_lib.BODY_ST_*`).  Values only: no graph (see `MassPropertiesFunction`)."""
    lib = _lib.load()
    kind, nverts = _raw(kind, "kind", torch.int32), _raw(nverts, "nverts", torch.int32)
    radius, verts_raw, mass = _raw(radius, "radius", torch.float64), _raw(verts_raw, "verts_raw", torch.float64), _raw(mass, "mass", torch.float64)
    B, nb, cap = verts_raw.shape[0], verts_raw.shape[1], verts_raw.shape[2]
    dev = verts_raw.device
    shapes = {"centroid": ((B, nb, 2), torch.float64), "verts_local": ((B, nb, cap, 2), torch.float64), "inertia": ((B, nb), torch.float64),
              "Mdiag": ((B, nb, 3), torch.float32), "f_gravity": ((B, nb, 3), torch.float32), "status": ((B, nb), torch.int32)}
    out = {k: torch.empty(s, dtype=d, device=dev) for k, (s, d) in shapes.items() if k in want}
    P = _lib.ptr
    with torch.cuda.device(dev):
        rc = lib.lcp_body_properties_f64(B, nb, cap, P(kind), P(radius), P(verts_raw), P(nverts), P(mass), float(g),
                                         *[P(out.get(k)) for k in shapes], _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_body_properties_f64")
    return out


def body_properties_backward(kind, radius, verts_raw, nverts, mass, g=0.0, g_centroid=None, g_verts_local=None, g_inertia=None,
                             g_Mdiag=None, g_f=None, want=("verts_raw", "radius", "mass")):
    """`lcp_body_properties_backward_f64`: the cotangents of the forward's outputs (None = zero) -> dict of d/d(verts_raw)
    [B,nb,cap,2], d/d(radius) [B,nb], d/d(mass) [B,nb] (f64) for the names in `want`."""
    lib = _lib.load()
    kind, nverts = _raw(kind, "kind", torch.int32), _raw(nverts, "nverts", torch.int32)
    radius, verts_raw, mass = _raw(radius, "radius", torch.float64), _raw(verts_raw, "verts_raw", torch.float64), _raw(mass, "mass", torch.float64)
    B, nb, cap = verts_raw.shape[0], verts_raw.shape[1], verts_raw.shape[2]
    dev = verts_raw.device
    cot = [None if t is None else _raw(t.contiguous(), n, d) for t, n, d in
           ((g_centroid, "g_centroid", torch.float64), (g_verts_local, "g_verts_local", torch.float64), (g_inertia, "g_inertia", torch.float64),
            (g_Mdiag, "g_Mdiag", torch.float32), (g_f, "g_f", torch.float32))]
    shapes = {"verts_raw": (B, nb, cap, 2), "radius": (B, nb), "mass": (B, nb)}
    out = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in shapes.items() if k in want}
    P = _lib.ptr
    with torch.cuda.device(dev):
        rc = lib.lcp_body_properties_backward_f64(B, nb, cap, P(kind), P(radius), P(verts_raw), P(nverts), P(mass), float(g),
                                                  *[P(t) for t in cot], *[P(out.get(k)) for k in shapes], _lib.stream_ptr(dev))
    _lib.check(rc, "lcp_body_properties_backward_f64")
    return out


class MassPropertiesFunction(torch.autograd.Function):
    """(radius, verts_raw, mass) -> (centroid, verts_local, inertia, Mdiag, f_gravity): one launch each way.

        centroid, verts_local, inertia, Mdiag, f_gravity = MassPropertiesFunction.apply(radius, verts_raw, mass, kind, nverts, g)

    `status` (optional, [B,nb] int32 on the device) receives the status words of the forward launch.  When none of the three inputs
    requires grad the outputs carry no backward node."""

    @staticmethod
    def forward(ctx, radius, verts_raw, mass, kind, nverts, g=0.0, status=None):
        out = body_properties(kind, radius, verts_raw, nverts, mass, g)
        if status is not None:
            status.copy_(out["status"])
        ctx.g = float(g)
        ctx.save_for_backward(radius, verts_raw, mass, kind, nverts)
        return out["centroid"], out["verts_local"], out["inertia"], out["Mdiag"], out["f_gravity"]

    @staticmethod
    def backward(ctx, g_centroid, g_verts_local, g_inertia, g_Mdiag, g_f):
        radius, verts_raw, mass, kind, nverts = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = tuple(n for n, k in (("radius", 0), ("verts_raw", 1), ("mass", 2)) if need[k])
        d = body_properties_backward(kind, radius, verts_raw, nverts, mass, ctx.g, g_centroid, g_verts_local, g_inertia, g_Mdiag, g_f,
                                     want=want)
        return d.get("radius"), d.get("verts_raw"), d.get("mass"), None, None, None, None


def _f64(a):
    return a.to(torch.float64) if isinstance(a, torch.Tensor) else torch.as_tensor(a, dtype=torch.float64)


@dataclass
class BodyBatch:
    """The bodies of B scenes, constructed on the device.  `geom`: a `GeometryBatch` whose `radius` and `verts_local` carry the graph
    of the raw shape; `p0` [B,nb,3] f64 = (rot, ref_point + centroid); `v0` [B,nb,3] f32; `Mdiag` [B,nb,3] f32 = (I, m, m);
    `f_gravity` [B,nb,3] f32 = (0, 0, m g) (zeros when g is None); `rest`, `fric` [B,nb] f32; `inertia` [B,nb] f64, `centroid`
    [B,nb,2] f64, `status` [B,nb] i32 (`_lib.BODY_ST_*`, on the device); `raw`: the launch's inputs (`raw_inputs`, on the device) -
    `raw["verts_raw"].retain_grad()` and the like give per-scene gradients where a learnable leaf is shared by the replicas."""
    geom: GeometryBatch
    p0: torch.Tensor
    v0: torch.Tensor
    Mdiag: torch.Tensor
    f_gravity: torch.Tensor
    rest: torch.Tensor
    fric: torch.Tensor
    inertia: torch.Tensor = None
    centroid: torch.Tensor = None
    status: torch.Tensor = None
    raw: dict = None

    @staticmethod
    def raw_inputs(bodies, B, max_verts=NV):
        """The inputs of the launch for `bodies` (see `from_list`), replicated B times, on the CPU: dict of kind, radius, verts_raw,
        nverts, mass, ref (rot, x, y of the reference point), v0, rest, fric.  A radius, dims, vertices, mass or pos given as a tensor
        that requires grad stays connected (autograd sums over the B replicas)."""
        nb = len(bodies)
        rows = []
        for b in bodies:
            k, pos, shape = b[0], b[1], b[2]
            opt = dict(b[3]) if len(b) > 3 else {}
            unknown = set(opt) - {"mass", "restitution", "fric_coeff", "vel"}
            if k not in ("circle", "rect", "hull") or unknown:
                raise ValueError("body %r: kind must be circle / rect / hull, options mass / restitution / fric_coeff / vel" % (b[:1] + tuple(unknown),))
            pos = _f64(pos).reshape(-1)
            if pos.numel() == 2:                                          # bodies.py:27-30
                pos = torch.cat([pos.new_zeros(1), pos])
            vel = _f64(opt.get("vel", (0.0, 0.0, 0.0))).reshape(-1)
            if vel.numel() == 2:                                          # bodies.py:36-39
                vel = torch.cat([vel.new_zeros(1), vel])
            rad, verts = torch.zeros((), dtype=torch.float64), None
            if k == "circle":
                rad = _f64(shape).reshape(())
            elif k == "rect":                                             # bodies.py:260-262
                half = _f64(shape).reshape(2) / 2
                v1 = half * half.new_tensor([-1.0, 1.0])
                verts = torch.stack([half, v1, -half, -v1])
            else:
                verts = torch.stack([_f64(v).reshape(2) for v in shape]) if isinstance(shape, (list, tuple)) else _f64(shape).reshape(-1, 2)
            rows.append((k, pos, vel, rad, verts, _f64(opt.get("mass", 1.0)).reshape(()), float(opt.get("restitution", RESTITUTION)),
                         float(opt.get("fric_coeff", FRIC_COEFF))))
        largest = max([r[4].shape[0] for r in rows if r[4] is not None], default=0)
        cap = max(NV, largest) if max_verts is None else int(max_verts)
        if not NV <= cap <= NV_MAX:
            raise ValueError("the vertex capacity must lie in [%d, %d] (got %d)" % (NV, NV_MAX, cap))
        if largest > cap:
            raise ValueError("hulls are limited to %d vertices" % cap)
        pad = lambda v: torch.zeros(cap, 2, dtype=torch.float64) if v is None else torch.cat([v, v.new_zeros(cap - v.shape[0], 2)])
        one = {"kind": torch.tensor([CIRCLE if r[0] == "circle" else HULL for r in rows], dtype=torch.int32),
               "radius": torch.stack([r[3] for r in rows]) if nb else torch.zeros(0, dtype=torch.float64),
               "verts_raw": torch.stack([pad(r[4]) for r in rows]) if nb else torch.zeros(0, cap, 2, dtype=torch.float64),
               "nverts": torch.tensor([0 if r[4] is None else r[4].shape[0] for r in rows], dtype=torch.int32),
               "mass": torch.stack([r[5] for r in rows]) if nb else torch.zeros(0, dtype=torch.float64),
               "ref": torch.stack([r[1] for r in rows]) if nb else torch.zeros(0, 3, dtype=torch.float64),
               "v0": (torch.stack([r[2] for r in rows]) if nb else torch.zeros(0, 3, dtype=torch.float64)).to(torch.float32),
               "rest": torch.tensor([r[6] for r in rows], dtype=torch.float32),
               "fric": torch.tensor([r[7] for r in rows], dtype=torch.float32)}
        rep = lambda t: t.unsqueeze(0).repeat(B, *([1] * t.dim())).contiguous()
        return {k: rep(t) for k, t in one.items()}

    @staticmethod
    def from_list(bodies, B, g=None, max_verts=NV, check=True, device="cuda"):
        """`bodies`: per body the reference's constructor arguments - ("circle", pos, rad, {options}), ("rect", pos, dims, {options}),
        ("hull", ref_point, verts, {options}); pos = (x, y) or (rot, x, y); options: mass (1), restitution (0.5), fric_coeff (0.9),
        vel ((0, 0, 0)) - replicated B times.  rad, dims, verts, mass and pos may be tensors that require grad (shared by the
        replicas).  `g`: `Gravity(g)` on every body (None: no gravity force).  `max_verts`: the vertex capacity, 8 .. 64 (None: the
        largest hull's).  `check`: read the status words once (ONE host synchronisation) and raise ValueError naming the first bad
        body; False: no synchronisation, `status` stays on the device.  `device`: where the launch runs (the inputs are built on the
        host, see `raw_inputs`, and moved there; `from_raw` starts from tensors that are on the device already)."""
        host = BodyBatch.raw_inputs(bodies, B, max_verts)
        svm = int(host["nverts"][0].sum()) if B else 0
        return BodyBatch.from_raw({k: t.to(device) for k, t in host.items()}, g=g, check=check, scene_verts_max=svm)

    @staticmethod
    def from_raw(raw, g=None, check=True, scene_verts_max=None):
        """`from_list` from the tensors of `raw_inputs`, already on the device: the launch, the optional status check and the assembly of
        the batch - device work only when `check` is False."""
        status = torch.empty(raw["kind"].shape, dtype=torch.int32, device=raw["kind"].device)
        centroid, verts_local, inertia, Mdiag, f_grav = MassPropertiesFunction.apply(
            raw["radius"], raw["verts_raw"], raw["mass"], raw["kind"], raw["nverts"], 0.0 if g is None else float(g), status)
        if check:
            BodyBatch.raise_on_status(status)
        geom = GeometryBatch(raw["kind"], raw["radius"], verts_local, raw["nverts"], None, scene_verts_max)
        p0 = raw["ref"] + torch.nn.functional.pad(centroid, (1, 0))                                  # bodies.py:173
        return BodyBatch(geom, p0, raw["v0"], Mdiag, f_grav, raw["rest"], raw["fric"], inertia, centroid, status, raw)

    @staticmethod
    def raise_on_status(status):
        """ValueError naming the first body whose status word is not 0 (synchronises)."""
        st = status.cpu()
        bad = st.reshape(-1).nonzero()
        if bad.numel():
            k = int(bad[0])
            word = int(st.reshape(-1)[k])
            raise ValueError("body %d of scene %d: %s (status %d)" % (k % st.shape[1], k // st.shape[1],
                                                                      "; ".join(t for bit, t in STATUS_NAMES if word & bit), word))

    def add_no_contact(self, i, j):
        """bodies.py:104-106: bodies i and j of every scene never collide."""
        g = self.geom
        if g.no_contact is None:
            g.no_contact = torch.zeros(g.B, g.nb, g.nb, dtype=torch.uint8, device=g.kind.device)
        g.no_contact[:, i, j] = 1
        g.no_contact[:, j, i] = 1
        return self

    def world(self, f=None, force_fn=None, **kw):
        """The `ContactWorld` of these bodies; `f` (constant, [B,nb,3]) or `force_fn(t)` are added to gravity."""
        from .batched_world import ContactWorld
        grav = self.f_gravity
        total = grav if f is None else grav + f.to(grav.dtype)
        fn = None if force_fn is None else (lambda t: total + force_fn(t).to(grav.dtype))
        return ContactWorld(self.geom, self.p0, self.v0, self.Mdiag, total, self.rest, self.fric, force_fn=fn, **kw)
