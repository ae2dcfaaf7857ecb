"""GPU: the buffer contract of every C entry point that takes a device pointer (include/lcp_hip.h), through the raw C ABI with all
buffers of a call sequence carved from one guarded arena (tests/guarded_buffers.py): exact sizes (a workspace of exactly
lcp_workspace_bytes), 256-byte alignment, a guard band around every buffer.

Per case: (a) the return codes are 0 or the code the routing table lists, (b) no guard byte changed, (c) every buffer a call does
not own as an output is bitwise unchanged across that call, (d) every element the header says is written is finite (the 0xFF fill
reads as NaN / -1) and the slots it says are zero are exactly zero, (e) a second run with guards and workspace prefilled with 0x00
and the buffers carved in reverse order gives bitwise the same outputs and tag, (f) runs with optional outputs NULL leave the
remaining outputs bitwise the same.  The cases are the rows of tests/test_device_routing.py (same scenes, compute and path words,
same tags) plus the sizes that table lacks, at the smallest batches that leave partial hardware units: B = 1 and 5 where four
scenes share a wavefront, B = 3 elsewhere.  Ragged contact counts: padded records zero against padded records NaN, bitwise."""
import numpy as np
import pytest
import torch

from tests.guarded_buffers import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
EPS, MAX_ITER, LIM = 1e-12, 10, 3
E_TOOLARGE = -2


class R(str):
    """An argument that is the device pointer of the arena buffer of this name (NULL when the buffer was not carved)."""


class Call:
    def __init__(self, fn, args, writes, rc=0):
        self.fn, self.args, self.writes, self.rc = fn, args, tuple(writes), rc


class Case:
    """bufs: [(name, dtype, shape, role, data)]; steps: Calls and python callables(arena); tag: the layout tag expected in `ws`;
    nulls: sets of optional buffers to leave out (one extra run each); post(outs): the zero-slot assertions;
    unwritten: {name: scenes whose rows the header does not promise}."""

    def __init__(self, B, bufs, steps, tag=None, nulls=(), post=None, unwritten=None):
        self.B, self.bufs, self.steps, self.tag, self.nulls, self.post = B, bufs, steps, tag, list(nulls), post
        self.unwritten = unwritten or {}


def _lib():
    from lcp_physics_amd import _lib as L
    return L


def _run(case, fill=0xFF, reverse=False, null=()):
    L = _lib()
    lib = L.load()
    ar = Arena(case.B, DEV, fill=fill, reverse=reverse)
    for name, dtype, shape, role, data in case.bufs:
        if name not in null:
            ar.add(name, dtype, shape, role=role, data=data)
    ar.build()
    stream = L.stream_ptr(torch.device(DEV))
    rcs = []
    for st in case.steps:
        if not isinstance(st, Call):
            st(ar)
            continue
        snap = ar.snapshot_inputs([n for n in ar.names() if n not in st.writes])
        rc = getattr(lib, st.fn)(*[ar.ptr(a) if isinstance(a, R) else a for a in st.args], stream)
        ar.sync()
        rcs.append(rc)
        assert rc == st.rc, (st.fn, "return code", rc, "expected", st.rc)                      # (a)
        viol = ar.check()
        assert viol == [], (st.fn, "guard bytes written (buffer, side, first, last)", viol)    # (b)
        changed = ar.inputs_unchanged(snap)
        assert changed == [], (st.fn, "buffers the call does not own were modified", changed)  # (c)
        if rc != 0:                                                                            # a refused call writes nothing
            for n in st.writes:
                if n in ar and ar.role(n) == "out":
                    assert bool((ar.bytes_of(n) == 0xFF).all()), (st.fn, n, "written by a call that returned", rc)
    outs = {n: ar[n].cpu().clone() for n in ar.names("out", "inout")}
    refused = {n for st in case.steps if isinstance(st, Call) and st.rc != 0 for n in st.writes}
    return outs, (ar.tag("ws") if "ws" in ar else None), refused


def _absmax(t):
    return float(t.double().abs().max()) if t.numel() else 0.0


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(U8), b.contiguous().view(-1).view(U8))


def _check(case):
    outs, tag, refused = _run(case)
    assert tag == case.tag, ("workspace tag", tag, "expected", case.tag)
    for n, t in outs.items():                                                                  # (d)
        if n in refused:
            continue
        keep = torch.ones(t.shape[0], dtype=torch.bool)
        for k in case.unwritten.get(n, ()):
            keep[k] = False
        t = t[keep]
        ok = torch.isfinite(t) if t.is_floating_point() else (t != -1)
        assert bool(ok.all()), (n, "elements not written / not finite", int((~ok).sum()), "first", (~ok).nonzero()[0].tolist())
    if "status" in outs and "status" not in refused:
        assert int((outs["status"] & _lib().ST_NAN).sum()) == 0, outs["status"].tolist()
    if case.post is not None:
        case.post(outs)
    again, tag2, _ = _run(case, fill=0x00, reverse=True)                                       # (e)
    assert tag2 == tag
    for n in outs:
        assert _same(outs[n], again[n]), (n, "depends on the neighbourhood of a buffer or on what the workspace held")
    for null in case.nulls:                                                                    # (f)
        part, _, _ = _run(case, null=frozenset(null))
        for n in part:
            assert _same(outs[n], part[n]), (n, "changes when", sorted(null), "are NULL")
    return outs


# ------------------------------------------------------------------------------------------------ contact-list scenes
def _scene(kind, B):
    from lcp_physics_amd import scenes
    if kind == "pile":                                       # BASELINE config 5: 11 bodies, 64 contacts
        return scenes.make_pile_scenes(B=B, seed=3, dtype=F32)
    if kind in ("stack", "joints6"):                         # 3 bodies, 8 contacts, the pinned floor / six general equality rows
        sc = scenes.make_stack_scenes(B=B, nbox=2, pts_per_interface=4, seed=7, dtype=F32)
        if kind == "joints6":
            sc.Je = torch.randn(B, 6, 3 * sc.nb, generator=torch.Generator().manual_seed(3)).float()
        return sc
    nbox, pts, e = kind
    sc = scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=900 + nbox + e, dtype=F32)
    if e > 3:                                                # chains: tests/test_hip_primal.py builds them like this
        from tests.test_hip_primal import _with_joint_rows
        sc = _with_joint_rows(sc, e)
    return sc


def _word(compute="f64", path="auto", pinned=False):
    L = _lib()
    arith = L.COMPUTE_F64 if compute == "f64" else L.COMPUTE_F32
    return arith, arith | L._PATH_BITS[path] | (L.HINT_PINNED if pinned else 0)


def _randn(seed, *shape, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


def _scene_bufs(sc, with_pos=True, with_f=True):
    B, nb, nc = sc.B, sc.nb, sc.nc
    e = sc.Je.shape[1]
    bufs = [("pos", F32, (B, nb, 3), "in", sc.p)] if with_pos else []
    bufs += [("Mdiag", F32, (B, nb, 3), "in", sc.Mdiag), ("v", F32, (B, nb, 3), "in", sc.v)]
    if with_f:
        bufs += [("f", F32, (B, nb, 3), "in", sc.f), ("fric", F32, (B, nb), "in", sc.fric)]
    bufs += [("rest", F32, (B, nb), "in", sc.rest), ("c_n", F32, (B, nc, 2), "in", sc.c_n), ("c_p1", F32, (B, nc, 2), "in", sc.c_p1),
             ("c_p2", F32, (B, nc, 2), "in", sc.c_p2), ("c_i1", I32, (B, nc), "in", sc.c_i1), ("c_i2", I32, (B, nc), "in", sc.c_i2)]
    if e:
        bufs.append(("Je", F32, (B, e, 3 * nb), "in", sc.Je))
    return bufs


_PHYS = ("Mdiag", "v", "f", "rest", "fric", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "Je")
_STEP_GRADS = ("dMdiag", "dv", "df", "drest", "dfric", "dc_n", "dc_p1", "dc_p2", "dJe")


def _grad_bufs(sc, names):
    B, nb, nc, e = sc.B, sc.nb, sc.nc, sc.Je.shape[1]
    shp = {"dMdiag": (B, nb, 3), "dv": (B, nb, 3), "df": (B, nb, 3), "drest": (B, nb), "dfric": (B, nb), "dc_n": (B, nc, 2),
           "dc_p1": (B, nc, 2), "dc_p2": (B, nc, 2), "dJe": (B, e, 3 * nb)}
    return [(n, F32, shp[n], "out", None) for n in names if n != "dJe" or e]


def _ws_bytes(B, nz, m, e, arith, io_f64=False):
    L = _lib()
    n = L.workspace_bytes(B, nz, m, e, arith | (L.IO_F64 if io_f64 else 0))
    assert n > 0
    return n


def _pad_rows(count, maxc):
    """[B, 4 maxc] mask of the rows of z / s that belong to padded contact slots ([normal | friction pairs | gamma] blocks)."""
    k = torch.arange(maxc).unsqueeze(0) >= count.long().unsqueeze(1)
    return torch.cat([k, k.repeat_interleave(2, dim=1), k], dim=1)


def _pad_slots(count, maxc):
    return torch.arange(maxc).unsqueeze(0) >= count.long().clamp(max=maxc).unsqueeze(1)


def _zero_pads(count, maxc, rows=("z", "s"), slots=("dc_n", "dc_p1", "dc_p2")):
    def post(outs):
        for n in rows:
            if n in outs:
                assert _absmax(outs[n][_pad_rows(count, maxc)]) == 0.0, (n, "padded rows are not zero")
        for n in slots:
            if n in outs:
                assert _absmax(outs[n][_pad_slots(count, maxc)]) == 0.0, (n, "padded slots are not zero")
    return post


def _step_case(kind, B, tag, compute="f64", path="auto", pinned=None, bwd_rc=0, count=None, je=True, sc=None):
    """lcp_step_fused_f32 (count None) or lcp_solve_dynamics_f32, then lcp_step_backward_je_f32 / lcp_step_backward_f32."""
    sc = _scene(kind, B) if sc is None else sc
    nb, nc, e = sc.nb, sc.nc, sc.Je.shape[1]
    if pinned is None:
        from lcp_physics_amd.physics.batched_world import rows_pin_leading_coordinates
        pinned = rows_pin_leading_coordinates(sc.Je)
    arith, word = _word(compute, path, pinned)
    fused = count is None
    bufs = _scene_bufs(sc, with_pos=fused)
    if not fused:
        bufs.append(("c_count", I32, (B,), "in", count))
    fwd_out = ["v_new"] + (["p_new"] if fused else []) + ["z", "s"] + (["y"] if e else []) + ["iters", "status"]
    shp = {"v_new": (B, nb, 3), "p_new": (B, nb, 3), "z": (B, 4 * nc), "s": (B, 4 * nc), "y": (B, e), "iters": (B,), "status": (B,)}
    bufs += [(n, I32 if n in ("iters", "status") else F32, shp[n], "out", None) for n in fwd_out]
    bufs.append(("ws", U8, (_ws_bytes(B, 3 * nb, 4 * nc, e, arith),), "ws", None))
    grads = [g for g in _STEP_GRADS if je or g != "dJe"]
    bufs.append(("dl_dv", F32, (B, nb, 3), "in", _randn(1, B, nb, 3)))
    bufs += _grad_bufs(sc, grads)
    phys = [R(n) for n in _PHYS]
    head = [B, nb, nc, e] + ([R("pos")] if fused else [R("c_count")])
    tail = [float(sc.dt), EPS, MAX_ITER, LIM, word, R("v_new")] + ([R("p_new")] if fused else []) + \
           [R("z"), R("s"), R("y"), R("iters"), R("status"), R("ws")]
    steps = [Call("lcp_step_fused_f32" if fused else "lcp_solve_dynamics_f32", head + phys + tail, fwd_out + ["ws"]),
             Call("lcp_step_backward_je_f32" if je else "lcp_step_backward_f32",
                  [B, nb, nc, e] + phys + [float(sc.dt), R("dl_dv"), word] + [R(g) for g in grads] + [R("ws")],
                  [g for g in grads] + ["ws"], rc=bwd_rc)]
    gl = [g for g in grads if g != "dJe" or e]
    nulls = [set(["z", "s", "y"]) | set(gl), set(gl[0::2]), set(gl[1::2])]
    cnt = torch.full((B,), nc, dtype=I32) if fused else count
    case = Case(B, bufs, steps, tag=tag, nulls=nulls, post=_zero_pads(cnt, nc))
    case.word = word
    return case


def _poststab_case(kind, B, tag, compute="f64", path="auto", count=None, pose="none", sc=None):
    """lcp_post_stabilization_f32 then its backward.  pose: "none" | "move" (p, dt_scene, p_out) | "alias" (p_out is p)."""
    sc = _scene(kind, B) if sc is None else sc
    nb, nc, e = sc.nb, sc.nc, sc.Je.shape[1]
    arith, word = _word(compute, path)
    count = torch.full((B,), nc, dtype=I32) if count is None else count
    bufs = _scene_bufs(sc, with_pos=False, with_f=False) + [("c_count", I32, (B,), "in", count)]
    outs = ["dp", "iters", "status"]
    p_arg = p_out_arg = dts_arg = None
    if pose != "none":
        p64 = sc.p.double() + 0.125
        bufs.append(("p", F64, (B, nb, 3), "inout" if pose == "alias" else "in", p64))
        bufs.append(("dt_scene", F64, (B,), "in", torch.full((B,), sc.dt, dtype=F64) / (1 + torch.arange(B, dtype=F64))))
        p_arg, dts_arg = R("p"), R("dt_scene")
        if pose == "alias":
            p_out_arg = R("p")
            outs.append("p")
        else:
            bufs.append(("p_out", F64, (B, nb, 3), "out", None))
            p_out_arg = R("p_out")
            outs.append("p_out")
    bufs += [("dp", F32, (B, nb, 3), "out", None), ("iters", I32, (B,), "out", None), ("status", I32, (B,), "out", None),
             ("ws", U8, (_ws_bytes(B, 3 * nb, 4 * nc, e, arith),), "ws", None), ("dl_ddp", F32, (B, nb, 3), "in", _randn(1, B, nb, 3))]
    grads = ["dMdiag", "dv", "drest", "dc_n", "dc_p1", "dc_p2", "dJe"]
    bufs += _grad_bufs(sc, grads)
    geo = [R(n) for n in ("Mdiag", "v", "rest", "c_n", "c_p1", "c_p2", "c_i1", "c_i2", "Je")]
    steps = [Call("lcp_post_stabilization_f32", [B, nb, nc, e, R("c_count")] + geo +
                  [EPS, MAX_ITER, LIM, word, p_arg, dts_arg, float(sc.dt), p_out_arg, R("dp"), R("iters"), R("status"), R("ws")],
                  outs + ["ws"]),
             Call("lcp_post_stabilization_backward_f32", [B, nb, nc, e] + geo + [R("dl_ddp"), word] + [R(g) for g in grads] + [R("ws")],
                  grads + ["ws"])]
    gl = [g for g in grads if g != "dJe" or e]
    nulls = [set(gl), set(gl[0::2]), set(gl[1::2])]
    if pose == "move":
        nulls.append({"p", "dt_scene", "p_out"})
    return Case(B, bufs, steps, tag=tag, nulls=nulls, post=_zero_pads(count, nc, rows=()))


_LCP = ("Q", "lp", "G", "h", "A", "b", "F")


def _lcp_bufs(B, nz, m, e, dtype, suffix="", prefix=""):
    shp = {"Q": (B, nz, nz), "lp": (B, nz), "G": (B, m, nz), "h": (B, m), "A": (B, e, nz), "b": (B, e), "F": (B, m, m)}
    return [(prefix + n + suffix, dtype, shp[n], "out", None) for n in _LCP if e or n not in ("A", "b")]


def _dense_case(kind, B, tag, compute="f64", path="auto", io_f64=False, perturb_A=False, bwd_rc=0):
    """lcp_assemble_contacts_f32, lcp_pdipm_forward_f32 / _f64 on what it wrote, then the dense backward."""
    sc = _scene(kind, B)
    nb, nc, e = sc.nb, sc.nc, sc.Je.shape[1]
    nz, m = 3 * nb, 4 * nc
    arith, word = _word(compute, path)
    dt_io, sfx = (F64, "64") if io_f64 else (F32, "")
    bufs = _scene_bufs(sc, with_pos=False) + _lcp_bufs(B, nz, m, e, F32)
    steps = [Call("lcp_assemble_contacts_f32", [B, nb, nc, e] + [R(n) for n in _PHYS] + [float(sc.dt)] + [R(n) for n in _LCP], _LCP)]
    if perturb_A:                                            # equality rows that do not pin the leading coordinates: class 3
        dA = 0.01 * torch.rand(B, e, nz, generator=torch.Generator().manual_seed(5))
        steps.append(lambda ar: ar["A"].add_(dA.to(DEV)))
    if io_f64:
        bufs += _lcp_bufs(B, nz, m, e, F64, suffix="64")
        steps.append(lambda ar: [ar[n + "64"].copy_(ar[n]) for n in _LCP if n in ar])
    sol = ["x", "y", "z", "s"]
    shp = {"x": (B, nz), "y": (B, e), "z": (B, m), "s": (B, m)}
    bufs += [(n, dt_io, shp[n], "out", None) for n in sol if e or n != "y"]
    bufs += [("iters", I32, (B,), "out", None), ("status", I32, (B,), "out", None),
             ("ws", U8, (_ws_bytes(B, nz, m, e, arith, io_f64),), "ws", None), ("dl_dx", dt_io, (B, nz), "in", _randn(2, B, nz))]
    grads = _lcp_bufs(B, nz, m, e, dt_io, prefix="d")
    bufs += grads
    gn = ["d" + n for n in _LCP]
    lcp_in = [R(n + sfx) for n in _LCP]
    steps.append(Call("lcp_pdipm_forward_f64" if io_f64 else "lcp_pdipm_forward_f32",
                      [B, nz, m, e] + lcp_in + [EPS, MAX_ITER, LIM] + ([] if io_f64 else [word]) +
                      [R(n) for n in sol] + [R("iters"), R("status"), R("ws")], sol + ["iters", "status", "ws"]))
    steps.append(Call("lcp_pdipm_backward_f64" if io_f64 else "lcp_pdipm_backward_f32",
                      [B, nz, m, e, R("G" + sfx), R("A" + sfx), R("dl_dx")] + ([] if io_f64 else [word]) + [R(g) for g in gn] + [R("ws")],
                      gn + ["ws"], rc=bwd_rc))
    gl = [g[0] for g in grads]
    return Case(B, bufs, steps, tag=tag, nulls=[set(gl), set(gl[0::2]), set(gl[1::2])])


def _all_contact_case(kind, B, tag, compute="f64", path="auto", bwd_rc=0):
    """The dense backward of a fused step (LCP_HINT_ALL_CONTACT) on the workspace the step left."""
    L = _lib()
    case = _step_case(kind, B, tag, compute=compute, path=path)
    sc = _scene(kind, B)
    nb, nc, e = sc.nb, sc.nc, sc.Je.shape[1]
    nz, m = 3 * nb, 4 * nc
    word = case.word
    names = {b[0] for b in case.bufs}
    bufs = [b for b in case.bufs if b[0] not in _STEP_GRADS and b[0] != "dl_dv"] + _lcp_bufs(B, nz, m, e, F32)
    grads = _lcp_bufs(B, nz, m, e, F32, prefix="g")          # (dp / dv of the step case are taken: the dense gradients are gQ, glp, ...)
    bufs += grads + [("dl_dx", F32, (B, nz), "in", _randn(2, B, nz))]
    assert not ({b[0] for b in grads} & names)
    gn = ["g" + n for n in _LCP]
    steps = [case.steps[0],
             Call("lcp_assemble_contacts_f32", [B, nb, nc, e] + [R(n) for n in _PHYS] + [float(sc.dt)] + [R(n) for n in _LCP], _LCP),
             Call("lcp_pdipm_backward_f32", [B, nz, m, e, R("G"), R("A"), R("dl_dx"), word | L.HINT_ALL_CONTACT] + [R(g) for g in gn] + [R("ws")],
                  gn + ["ws"], rc=bwd_rc)]
    gl = [g[0] for g in grads]
    return Case(B, bufs, steps, tag=tag, nulls=[set(gl), set(gl[0::2])])


# ------------------------------------------------------------------------------------------------ the routing table
QUAD_B, B3 = (1, 5), (3,)        # four scenes share a wavefront: one full wave plus a quarter-filled one; three scenes elsewhere
ROUTES = [
    # the rows of tests/test_device_routing.py::CASES: (case, builder, keywords, tag, batch sizes)
    ("step quad body", _step_case, dict(kind="stack"), 4, QUAD_B),
    ("step quad contact space", _step_case, dict(kind="stack", path="big"), 5, QUAD_B),
    ("step quad fp32", _step_case, dict(kind="stack", compute="f32"), 5, QUAD_B),
    ("step quad forced", _step_case, dict(kind="stack", path="quad"), 4, QUAD_B),
    ("step solo forced", _step_case, dict(kind="stack", path="solo"), 4, B3),
    ("step quad unpinned", _step_case, dict(kind="stack", pinned=False), 4, QUAD_B),
    ("step generic", _step_case, dict(kind="stack", path="generic"), 9, B3),
    ("step primal forced", _step_case, dict(kind="stack", path="primal"), 6, B3),
    ("step primal_wg forced", _step_case, dict(kind="stack", path="primal_wg"), 13, B3),
    ("step primal pinned", _step_case, dict(kind="pile"), 6, B3),
    ("step primal unpinned", _step_case, dict(kind="pile", pinned=False), 6, B3),
    ("step big", _step_case, dict(kind="pile", path="big"), 7, B3),
    ("step fp32 generic", _step_case, dict(kind="pile", compute="f32"), 9, B3),
    ("step primal_wg pinned", _step_case, dict(kind="pile", path="primal_wg"), 13, B3),
    ("step wave64", _step_case, dict(kind="joints6", compute="f32", bwd_rc=E_TOOLARGE), 8, B3),
    ("counts quad", _step_case, dict(kind="stack", pinned=True, count="full", je=False), 4, QUAD_B),
    ("counts primal", _step_case, dict(kind="pile", pinned=True, count="full", je=False), 6, B3),
    ("counts primal_wg", _step_case, dict(kind="pile", path="primal_wg", pinned=True, count="full", je=False), 13, B3),
    ("counts wave64 sizes: generic", _step_case, dict(kind="joints6", compute="f32", pinned=False, count="full", bwd_rc=E_TOOLARGE), 9, B3),
    ("poststab quad", _poststab_case, dict(kind="stack", pose="move"), 10, QUAD_B),
    ("poststab primal forced", _poststab_case, dict(kind="stack", path="primal", pose="alias"), 10, B3),
    ("poststab primal", _poststab_case, dict(kind="pile"), 10, B3),
    ("poststab generic", _poststab_case, dict(kind="stack", path="generic", pose="move"), 11, B3),
    ("poststab fp32", _poststab_case, dict(kind="pile", compute="f32"), 11, B3),
    ("dense wave64 quad body", _dense_case, dict(kind="stack"), 12, QUAD_B),
    ("dense wave64 contact space", _dense_case, dict(kind="stack", path="big"), 1, QUAD_B),
    ("dense wave64 fp32", _dense_case, dict(kind="stack", compute="f32"), 1, QUAD_B),
    ("dense wave64 wave", _dense_case, dict(kind="joints6"), 1, B3),
    ("dense generic", _dense_case, dict(kind="stack", path="generic"), 3, B3),
    ("dense fp64 io", _dense_case, dict(kind="stack", io_f64=True), 1, B3),
    ("dense big primal class 4", _dense_case, dict(kind="pile"), 2, B3),
    ("dense big primal class 3", _dense_case, dict(kind="pile", perturb_A=True), 2, B3),
    ("dense big contact space", _dense_case, dict(kind="pile", path="big"), 2, B3),
    ("dense fp32 generic", _dense_case, dict(kind="pile", compute="f32"), 3, B3),
    ("dense fp64 io generic sizes", _dense_case, dict(kind="pile", io_f64=True), 3, B3),
    ("all-contact quad body", _all_contact_case, dict(kind="stack"), 4, QUAD_B),
    ("all-contact quad contact space", _all_contact_case, dict(kind="stack", path="big"), 5, QUAD_B),
    ("all-contact generic", _all_contact_case, dict(kind="stack", path="generic"), 9, B3),
    ("all-contact primal", _all_contact_case, dict(kind="pile", bwd_rc=E_TOOLARGE), 6, B3),
    # sizes the table lacks.  The sized four-scenes-per-wave instantiations (_n6e3 .. _n15e3): 1 .. 4 boxes on the pinned floor
    ("size quad n6e3", _step_case, dict(kind=(1, 4, 3), path="quad", pinned=True), 4, QUAD_B),
    ("size quad n9e3", _step_case, dict(kind=(2, 4, 3), path="quad", pinned=True), 4, QUAD_B),
    ("size quad n12e3", _step_case, dict(kind=(3, 4, 3), path="quad", pinned=True), 4, QUAD_B),
    ("size quad n15e3", _step_case, dict(kind=(4, 4, 3), path="quad", pinned=True), 4, QUAD_B),
    # chains of joints on lcp_primal_chain.hip: 7 and 24 equality rows
    ("size chain e7", _step_case, dict(kind=(4, 2, 7)), 6, B3),
    ("size chain e24", _step_case, dict(kind=(8, 2, 24)), 6, B3),
    # the 64-row body-space instantiation: 20 bodies on the pinned floor
    ("size primal 20 bodies", _step_case, dict(kind=(19, 1, 3), pinned=True), 6, B3),
    # one workgroup per scene: 20 bodies forced, and its largest pinned size (43 bodies: 126 pivots)
    ("size primal_wg 20 bodies", _step_case, dict(kind=(19, 1, 3), path="primal_wg", pinned=True), 13, B3),
    ("size primal_wg 43 bodies", _step_case, dict(kind=(42, 1, 3), pinned=True), 13, B3),
    # the generic kernels beyond 64 contacts (fp32 arithmetic: in fp64 these sizes belong to the workgroup-per-scene kernel)
    ("size generic 66 contacts", _step_case, dict(kind=(11, 6, 3), compute="f32"), 9, B3),
]
_ROUTE_PARAMS = [pytest.param(fn, dict(kw), tag, B, id="%s-B%d" % (name, B)) for name, fn, kw, tag, Bs in ROUTES for B in Bs]


def test_the_cases_cover_the_routing_table():
    from tests.test_device_routing import CASES
    mine = {r[0]: r[3] for r in ROUTES}
    assert [(c[0], c[2]) for c in CASES] == [(c[0], mine.get(c[0])) for c in CASES]
    codes = {"finite": 0, "LCP_E_TOOLARGE": E_TOOLARGE}
    assert [codes[c[3]] for c in CASES] == [r[2].get("bwd_rc", 0) for r in ROUTES[:len(CASES)]]


@pytest.mark.parametrize("fn,kw,tag,B", _ROUTE_PARAMS)
def test_route_buffer_contract(fn, kw, tag, B):
    if kw.get("count") == "full":
        kw["count"] = torch.full((B,), _scene(kw["kind"], B).nc, dtype=I32)
    _check(fn(B=B, tag=tag, **kw))


# ------------------------------------------------------------------------------------------------ ragged contact counts
def _ragged_counts(maxc):
    return torch.tensor([0, 1, maxc, maxc // 2, maxc - 1], dtype=I32)


def _poison_padding(sc, count, value):
    """The float fields of the records beyond each scene's count set to `value`; the padded body indices stay valid."""
    from dataclasses import replace
    pad = _pad_slots(count, sc.nc)
    kw = {}
    for n in ("c_n", "c_p1", "c_p2"):
        t = getattr(sc, n).clone()
        t[pad] = value
        kw[n] = t
    return replace(sc, **kw)


RAGGED = [
    ("solve_dynamics quad", _step_case, dict(kind="stack", path="quad", pinned=True), 4),
    ("solve_dynamics solo", _step_case, dict(kind="stack", path="solo", pinned=True), 4),
    ("solve_dynamics body-space", _step_case, dict(kind="pile", pinned=True), 6),
    ("solve_dynamics contact-space big", _step_case, dict(kind="pile", path="big"), 7),
    ("solve_dynamics workgroup", _step_case, dict(kind="pile", path="primal_wg", pinned=True), 13),
    ("solve_dynamics generic", _step_case, dict(kind="stack", path="generic"), 9),
    ("post_stabilization quad", _poststab_case, dict(kind="stack"), 10),
    ("post_stabilization body-space", _poststab_case, dict(kind="pile"), 10),
    ("post_stabilization generic", _poststab_case, dict(kind="stack", path="generic"), 11),
]


@pytest.mark.parametrize("name,fn,kw,tag", RAGGED, ids=[r[0] for r in RAGGED])
def test_ragged_counts_never_read_the_padding(name, fn, kw, tag):
    """Counts [0, 1, maxc, maxc / 2, maxc - 1] over B = 5: the outputs with NaN in the float fields of the padded records are bitwise
    those with zeros there, padded rows of z / s and padded gradient slots are exactly zero, guards intact."""
    B = 5
    sc = _scene(kw["kind"], B)
    count = _ragged_counts(sc.nc)
    extra = dict(je=False) if fn is _step_case else {}
    outs = {}
    for value in (0.0, float("nan")):
        case = fn(B=B, tag=tag, count=count, sc=_poison_padding(sc, count, value), **extra, **kw)
        case.nulls = []
        outs[value == 0.0] = _check(case)
    for n in outs[True]:
        assert _same(outs[True][n], outs[False][n]), (n, "depends on the padded records")


# ------------------------------------------------------------------------------------------------ narrow phase
def _geometry(scenes_, nvcap):
    """(kind, radius, verts_local, nverts, pose, per-scene vertex totals) on the CPU for a list of (shapes, pose[nb,3])."""
    from lcp_physics_amd.physics.contacts import GeometryBatch
    gs = [GeometryBatch.from_shapes(sh, 1, max_verts=nvcap) for sh, _ in scenes_]
    cat = lambda k: torch.cat([getattr(g, k) for g in gs])
    pose = torch.tensor(np.stack([p for _, p in scenes_]), dtype=F64)
    return cat("kind"), cat("radius"), cat("verts_local"), cat("nverts"), pose, [g.scene_verts_max for g in gs]


def _contacts_case(scenes_, maxc, nvcap=8, wide=False, move=False, svm=None, bad=(), no_contact=False):
    """Detection, the pose backward of the contact frame, then the shape backward, on the records the detection wrote."""
    kind, radius, verts, nverts, pose, totals = _geometry(scenes_, nvcap)
    B, nb = pose.shape[0], pose.shape[1]
    svm = max(totals) if svm is None else svm
    bufs = [("kind", I32, (B, nb), "in", kind), ("radius", F64, (B, nb), "in", radius), ("verts_local", F64, (B, nb, nvcap, 2), "in", verts),
            ("nverts", I32, (B, nb), "in", nverts), ("p_start", F64, (B, nb, 3), "in", pose)]
    if no_contact:
        mask = torch.zeros(B, nb, nb, dtype=U8)
        mask[B - 1, 0, 1] = mask[B - 1, 1, 0] = 1
        bufs.append(("no_contact", U8, (B, nb, nb), "in", mask))
    if move:
        v = torch.zeros(B, nb, 3)
        v[:, 1:, 2] = 40.0 + 10.0 * torch.arange(B).reshape(B, 1)
        bufs.append(("v", F32, (B, nb, 3), "in", v))
    det = [("p_out", F64, (B, nb, 3)), ("c_n", F32, (B, maxc, 2)), ("c_p1", F32, (B, maxc, 2)), ("c_p2", F32, (B, maxc, 2)),
           ("c_pen", F64, (B, maxc)), ("c_i1", I32, (B, maxc)), ("c_i2", I32, (B, maxc)), ("count", I32, (B,)), ("max_pen", F64, (B,)),
           ("dt_used", F64, (B,)), ("trials", I32, (B,))]
    bufs += [(n, d, s, "out", None) for n, d, s in det] + [("t", F64, (B,), "inout", torch.zeros(B, dtype=F64))]
    bufs += [("g_n", F32, (B, maxc, 2), "in", _randn(11, B, maxc, 2)), ("g_p1", F32, (B, maxc, 2), "in", _randn(12, B, maxc, 2)),
             ("g_p2", F32, (B, maxc, 2), "in", _randn(13, B, maxc, 2)), ("dpose", F64, (B, nb, 3), "out", None),
             ("d_radius", F64, (B, nb), "out", None), ("d_verts_local", F64, (B, nb, nvcap, 2), "out", None)]
    geo = [R("kind"), R("radius"), R("verts_local"), R("nverts")]
    dt = 1.0 / 30
    sizes = [B, nb, maxc] + ([nvcap, svm] if wide else [])
    pose_at = R("p_out") if move else R("p_start")           # (v = NULL detects at p_start itself)
    steps = [Call("lcp_move_find_contacts_nv_f64" if wide else "lcp_move_find_contacts_f64",
                  sizes + geo + [R("no_contact"), R("p_start"), R("v"), dt, dt / 4, 1, 16 if move else 1, 0.1, 1e-6] +
                  [R(n) for n in ("p_out", "c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2", "count", "max_pen", "dt_used", "t", "trials")],
                  [n for n, _, _ in det] + ["t"])]
    grads = [R("g_n"), R("g_p1"), R("g_p2")]
    if wide:
        steps.append(Call("lcp_contact_frame_backward_nv_f64", sizes + geo + [R("no_contact"), pose_at, 0.1, R("count"), R("c_i1"), R("c_i2")] +
                          grads + [R("dpose")], ["dpose"]))
    else:
        steps.append(Call("lcp_contact_frame_backward_f64", sizes + geo + [R("no_contact"), pose_at, 0.1, R("count")] + grads + [R("dpose")],
                          ["dpose"]))
    steps.append(Call("lcp_contact_frame_backward_shape_f64", [B, nb, maxc, nvcap, svm] + geo + [pose_at, 0.1, R("count"), R("c_i1"), R("c_i2")] +
                      grads + [R("d_radius"), R("d_verts_local")], ["d_radius", "d_verts_local"]))
    opt = {"c_pen", "max_pen", "dt_used", "t", "trials"} | (set() if move else {"p_out"})
    bad = list(bad)
    unwritten = {n: bad for n in ("p_out", "count", "max_pen", "dt_used", "trials", "t")}

    def post(outs):
        cnt = outs["count"]
        good = [k for k in range(B) if k not in bad]
        assert cnt[bad].tolist() == [-1] * len(bad) and bool((cnt[good] >= 0).all()), cnt.tolist()
        pad = _pad_slots(cnt.clamp(min=0), maxc)
        for n in ("c_n", "c_p1", "c_p2", "c_pen", "c_i1", "c_i2"):
            assert _absmax(outs[n][pad]) == 0.0, (n, "padded records are not zero")
        slot = torch.arange(nvcap).reshape(1, 1, nvcap) >= torch.where(kind == 0, torch.zeros_like(nverts), nverts).unsqueeze(2)
        assert _absmax(outs["d_verts_local"][slot]) == 0.0, "vertex slots >= nverts (and circles) are not zero"
        assert _absmax(outs["d_radius"][kind != 0]) == 0.0, "hulls have a radius gradient"
        for k in bad:                                        # the over-capacity scene: zeros throughout
            assert float(outs["d_radius"][k].abs().max()) == 0.0 and float(outs["d_verts_local"][k].abs().max()) == 0.0
        return cnt

    return Case(B, bufs, steps, nulls=[opt, {"d_radius"}, {"d_verts_local"}], post=post, unwritten=unwritten)


def _narrow_scenes(nb, B, seed):
    from tests.test_hip_contacts import _random_scene
    rng = np.random.default_rng(seed)
    return [_random_scene(rng, nb) for _ in range(B)]


def _wide_scenes(nb, B, seed, nvr):
    from tests.test_hip_wide_contacts import _wide_scene
    rng = np.random.default_rng(seed)
    return [_wide_scene(rng, nb, nv_range=nvr) for _ in range(B)]


@pytest.mark.parametrize("B", QUAD_B)
def test_narrow_detection_3_bodies(B):
    """lcp_move_find_contacts_f64 with the move and dt halving (four scenes per wave at these sizes), the pose and the shape backward."""
    outs = _check(_contacts_case(_narrow_scenes(3, B, 7), maxc=16, no_contact=True, move=True))
    assert B == 1 or int(outs["count"].max()) > 0            # (B = 1 is the scene whose floor contact the mask removes)


def test_narrow_detection_overflows_maxc():
    """nb = 5, v = NULL, with maxc below one scene's list: count > maxc is reported, nothing is written past slot maxc - 1 (the guards),
    and the backwards use the first maxc records only."""
    sc = _narrow_scenes(5, 3, 3)
    full = _check(_contacts_case(sc, maxc=16))["count"]
    maxc = int(full.max()) - 1
    assert maxc >= 1
    outs = _check(_contacts_case(sc, maxc=maxc))
    assert outs["count"].tolist() == full.tolist() and int(outs["count"].max()) > maxc


def test_wide_detection_33_bodies_capacity_16():
    outs = _check(_contacts_case(_wide_scenes(33, 3, 2064, (9, 17)), maxc=128, nvcap=16, wide=True, move=True))
    assert int(outs["count"].min()) > 0


def test_wide_detection_12_bodies_capacity_64_with_a_scene_over_scene_verts_max():
    """v = NULL; scene_verts_max is the second largest vertex total: the largest scene gets count = -1, no records, and zero
    shape gradients."""
    sc = _wide_scenes(12, 3, 2065, (9, 65))
    totals = _geometry(sc, 64)[5]
    order = sorted(range(3), key=lambda k: totals[k])
    assert totals[order[2]] > totals[order[1]]
    outs = _check(_contacts_case(sc, maxc=48, nvcap=64, wide=True, svm=totals[order[1]], bad=[order[2]]))
    assert int(outs["count"].max()) > 0


@pytest.mark.parametrize("entry", ["narrow", "wide", "shape"])
def test_frame_backwards_never_read_the_padding(entry):
    """The three frame backwards over B = 5 scenes with counts [0, 1, maxc, maxc / 2, ..]: cotangents and records beyond each scene's
    count zero against NaN (the padded body indices stay valid), bitwise the same gradients."""
    B, nb, nvcap = 5, 5, (8 if entry != "wide" else 16)
    det = _contacts_case(_narrow_scenes(nb, B, 21), maxc=16, nvcap=nvcap, wide=entry == "wide")
    found = _check(det)
    maxc = int(found["count"].max())
    assert maxc >= 2
    count = torch.minimum(found["count"], torch.tensor([0, 1, maxc, maxc // 2, maxc], dtype=I32))
    pad = _pad_slots(count, maxc)
    res = {}
    for value in (0.0, float("nan")):
        bufs = [b for b in det.bufs if b[3] == "in" and b[0] not in ("g_n", "g_p1", "g_p2")]
        bufs.append(("count", I32, (B,), "in", count))
        for n, seed in (("g_n", 11), ("g_p1", 12), ("g_p2", 13)):
            g = _randn(seed, B, maxc, 2)
            g[pad] = value
            bufs.append((n, F32, (B, maxc, 2), "in", g))
        for n in ("c_i1", "c_i2"):
            bufs.append((n, I32, (B, maxc), "in", torch.where(pad, torch.zeros_like(found[n][:, :maxc]), found[n][:, :maxc])))
        geo = [R("kind"), R("radius"), R("verts_local"), R("nverts")]
        gr = [R("g_n"), R("g_p1"), R("g_p2")]
        svm = det.steps[2].args[4]
        if entry == "narrow":
            bufs.append(("dpose", F64, (B, nb, 3), "out", None))
            call = Call("lcp_contact_frame_backward_f64", [B, nb, maxc] + geo + [None, R("p_start"), 0.1, R("count")] + gr + [R("dpose")], ["dpose"])
        elif entry == "wide":
            bufs.append(("dpose", F64, (B, nb, 3), "out", None))
            call = Call("lcp_contact_frame_backward_nv_f64", [B, nb, maxc, nvcap, svm] + geo +
                        [None, R("p_start"), 0.1, R("count"), R("c_i1"), R("c_i2")] + gr + [R("dpose")], ["dpose"])
        else:
            bufs += [("d_radius", F64, (B, nb), "out", None), ("d_verts_local", F64, (B, nb, nvcap, 2), "out", None)]
            call = Call("lcp_contact_frame_backward_shape_f64", [B, nb, maxc, nvcap, svm] + geo +
                        [R("p_start"), 0.1, R("count"), R("c_i1"), R("c_i2")] + gr + [R("d_radius"), R("d_verts_local")],
                        ["d_radius", "d_verts_local"])
        res[value == 0.0] = _check(Case(B, bufs, [call]))
    for n in res[True]:
        assert _same(res[True][n], res[False][n]), (n, "depends on the padded records")
        assert float(res[True][n][0].abs().max()) == 0.0, (n, "a scene without contacts has a gradient")


# ------------------------------------------------------------------------------------------------ joints and the state update
def _joint_case(B, move):
    from lcp_physics_amd.physics.joints import JointSet
    nb = 4
    p0 = torch.zeros(nb, 3, dtype=F64)
    p0[:, 1] = 300.0
    p0[:, 2] = 50.0 + 50.0 * torch.arange(nb, dtype=F64)
    js = JointSet.from_list([("joint", 0, None, (300.0, 30.0)), ("joint", 1, 0, (300.0, 75.0)), ("fixed", 2, 1), ("x", 3), ("rot", 3),
                             ("total", 3)], p0, B=B)
    nj, e = js.jtype.shape[1], js.e
    pose = p0.unsqueeze(0).repeat(B, 1, 1) + 0.01 * _randn(4, B, nb, 3, dtype=F64)
    bufs = [("jtype", I32, (B, nj), "in", js.jtype), ("jb1", I32, (B, nj), "in", js.jb1), ("jb2", I32, (B, nj), "in", js.jb2),
            ("jr1", F64, (B, nj), "in", js.jr1), ("jrot1", F64, (B, nj), "inout", js.jrot1), ("p", F64, (B, nb, 3), "in", pose),
            ("Je", F32, (B, e, 3 * nb), "out", None), ("gJe", F32, (B, e, 3 * nb), "in", _randn(5, B, e, 3 * nb)),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_rot", F64, (B, nj), "out", None),
            ("gp_in", F64, (B, nb, 3), "in", _randn(6, B, nb, 3, dtype=F64)), ("gg_in", F64, (B, nb, 3), "in", _randn(7, B, nb, 3, dtype=F64)),
            ("grot_in", F64, (B, nj), "in", _randn(8, B, nj, dtype=F64)), ("g_v", F32, (B, nb, 3), "out", None)]
    if move:
        bufs += [("v", F32, (B, nb, 3), "in", _randn(9, B, nb, 3)),
                 ("dt_scene", F64, (B,), "in", (1.0 / 30) / (1 + torch.arange(B, dtype=F64)))]
    else:                                                    # the state update always needs the velocities and the accepted dt
        bufs += [("v_su", F32, (B, nb, 3), "in", _randn(9, B, nb, 3)), ("dt_su", F64, (B,), "in", torch.full((B,), 1.0 / 30, dtype=F64))]
    ids = [R("jtype"), R("jb1"), R("jb2"), R("jr1")]
    jac_writes = ["Je"] + (["jrot1"] if move else [])        # (jrot1 is in-out only when the joints are moved: v != NULL)
    steps = [Call("lcp_joint_jacobian_f64", [B, nb, nj, e] + ids + [R("jrot1"), R("p"), R("v"), R("dt_scene"), 1.0 / 30, 1.0, R("Je")], jac_writes),
             Call("lcp_joint_jacobian_backward_f64", [B, nb, nj, e] + ids + [R("jrot1"), R("gJe"), R("g_p"), R("g_rot")], ["g_p", "g_rot"]),
             Call("lcp_state_update_backward_f64", [B, nb, nj, R("gp_in"), R("gg_in"), R("grot_in"), R("v" if move else "v_su"),
                                                    R("dt_scene" if move else "dt_su"), 0.5, R("jtype"), R("jb1"), R("g_v")], ["g_v"])]
    return Case(B, bufs, steps, nulls=[{"gp_in"}, {"gg_in"}, {"grot_in"}, {"gp_in", "gg_in", "grot_in"}] if not move else [])


@pytest.mark.parametrize("move", [False, True], ids=["at-pose", "moved"])
def test_joint_jacobian_and_state_update(move):
    """lcp_joint_jacobian_f64 (jrot1 in-out when the joints move, const otherwise), its backward (g_p written, not accumulated) and
    lcp_state_update_backward_f64 with each optional cotangent NULL."""
    case = _joint_case(3, move)
    if not move:                                             # a NULL cotangent changes g_v: only guards and codes are checked there
        nulls, case.nulls = case.nulls, []
        _check(case)
        for null in nulls:
            _run(case, null=frozenset(null))
        return
    outs = _check(case)
    jrot0 = [b for b in case.bufs if b[0] == "jrot1"][0][4]
    assert not torch.equal(outs["jrot1"], jrot0)             # the revolute joints were advanced in place ...
    assert torch.equal(outs["jrot1"][:, 2:], jrot0[:, 2:])   # ... and only those
