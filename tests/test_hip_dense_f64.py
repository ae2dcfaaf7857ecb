"""Dense fp64 boundary: `lcp_pdipm_forward_f64` / `lcp_pdipm_backward_f64` (what `LCPFunction` runs on fp64 tensors, the
reference's default dtype) on UNSTRUCTURED LCPs, against the oracle on the identical fp64 inputs.

An unstructured LCP is the only input that reaches the general branch of the wave-per-scene family (`lcp_*_wave_any`, partial
pivoting) and the `<double, double>` instantiations of the generic kernels.  Random monotone dense LCPs
(`scenes.make_random_lcp`) are conditioned to rounding: `test_oracle_agrees_with_itself_under_reordering` (host only) solves every
shape of this module a second time with its unknowns and rows in another order and holds the oracle to 1e-10 of itself (measured:
<= 1.3e-13 forward, <= 2.1e-13 on every gradient, equal iteration counts).  So NO mask is applied anywhere below, and the
project's fp64-I/O gates (1e-7 on the solution, 1e-6 on the seven gradients: tests/test_hip_parity.py, DESIGN numerics 4) sit six
orders above the reference's own noise - a kernel that is slightly wrong cannot pass them.

Limits read from the code: `wave64_supported` nz <= 16, m <= 64, e <= 8 (lcp_wave_common.h NZP / MP / EP); `quad_supported`
m % 4 == 0, m / 4 <= 16, nz <= 16, e <= 4 (the four-scenes-per-wave launch runs first and `lcp_*_wave_any` skips its scenes: on
unstructured input every scene must still reach the general body); `make_plan(nz, m, e, 8)` with 160 KiB of LDS: level 1
(everything in LDS), level 0 (T and the prefactor scratch in the workspace), level 2 (Q, Q^-1 and G there too).

Measured on an MI355X (largest value over the scenes and over max_iter 10 and 20; "fwd" = worst of x, z, s, y; "grad" = worst of
the seven gradients; plain per-scene relative errors, `parity.rel_err`):

                     library's choice              generic kernels forced
    (nz, m, e)       tag   fwd       grad          tag   fwd       grad
    (6, 4, 3)        1     1.9e-13   3.7e-13       3     1.7e-13   3.3e-13
    (9, 32, 3)       1     2.9e-15   1.6e-14       3     1.5e-15   1.2e-14
    (15, 64, 3)      1     1.4e-15   1.2e-13       3     9.5e-16   1.0e-13
    (16, 64, 8)      1     1.1e-15   3.5e-12       3     2.0e-15   3.6e-12
    (7, 23, 0)       1     1.8e-15   2.5e-15       3     8.4e-16   3.5e-15
    (1, 1, 0)        1     4.0e-13   2.5e-13       3     4.0e-13   2.5e-13
    (16, 64, 0)      1     7.3e-16   1.0e-14       3     9.8e-16   3.4e-15
    (17, 64, 3)      3     1.4e-15   7.9e-15       3     1.4e-15   7.9e-15
    (16, 65, 0)      3     8.5e-16   6.2e-15       3     8.5e-16   6.2e-15
    (16, 64, 9)      3     3.0e-15   2.2e-14       3     3.0e-15   2.2e-14
    (20, 96, 2)      3     1.6e-15   1.0e-14       3     1.6e-15   1.0e-14
    (12, 130, 1)     3     4.7e-14   2.1e-14       3     4.7e-14   2.1e-14
    (84, 64, 2)      3     2.6e-15   2.5e-14       3     2.6e-15   2.5e-14
    mixed batch (15, 64, 3), unstructured scenes:
                     1     1.4e-15   1.2e-13       3     6.7e-16   1.1e-13

(tag 1 = TAG_DENSE_WAVE, 3 = TAG_DENSE_GENERIC.)  Every figure is five orders or more inside its gate; the largest, 3.6e-12 on the
gradients of (16, 64, 8) at max_iter 20 (a converged solve with eight equality rows), shows on both kernel families alike.
Each test prints its own figures (`pytest -s`).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import pdipm_oracle as O
from tests import parity

DEV = "cuda"
B = 8
TOL_X64 = 1e-7           # the project's fp64-I/O gate on the solution
TOL_G64 = 1e-6           # ... and on the gradients
TOL_SELF = 1e-10         # the oracle against itself in another elimination order (host test)
TAG_DENSE_WAVE, TAG_DENSE_GENERIC = 1, 3                 # lcp_api.cpp WsTag
WAVE_NZ, WAVE_M, WAVE_E = 16, 64, 8                      # wave64_supported
GRAD_KEYS = "QpGhAbF"

# (nz, m, e): what the shape is there for
SHAPES = [
    # inside the wave-per-scene family
    (6, 4, 3),        # one contact's worth of rows; quad_supported sizes
    (9, 32, 3),       # quad_supported sizes
    (15, 64, 3),      # the shape of the mixed batches below; quad_supported sizes
    (16, 64, 8),      # all three limits at once (e > 4: no four-scenes-per-wave launch)
    (7, 23, 0),       # m no multiple of 4; no equality rows: A, b absent
    (1, 1, 0),        # the smallest LCP there is
    (16, 64, 0),      # both size limits without equality rows
    # one step outside each limit: the generic kernels, make_plan level 1
    (17, 64, 3),
    (16, 65, 0),
    (16, 64, 9),
    # the generic plan levels with 8-byte elements (LDS bytes of make_plan(nz, m, e, 8))
    (20, 96, 2),      # level 1: 126912 bytes, everything in LDS
    (12, 130, 1),     # level 0: level 1 would need 181 KB; T (130 x 131) and the scratch in the workspace, 32976 bytes of LDS
    (84, 64, 2),      # level 2: level 0 would need 167 KB; Q, Q^-1, G in the workspace too, 15936 bytes of LDS
]
PLAN_LEVEL = {(20, 96, 2): 1, (12, 130, 1): 0, (84, 64, 2): 2}
MAX_ITERS = [10, 20]     # 10 (the default): these solves stop at the limit; 20: they converge
_id = lambda s: "nz%d_m%d_e%d" % s


def _in_wave_family(nz, m, e):
    return nz <= WAVE_NZ and m <= WAVE_M and e <= WAVE_E


@pytest.fixture(params=["auto", "generic"])
def route(request):
    """The library's own choice of kernels, then the generic kernels forced; the calling thread's default is restored."""
    from lcp_physics_amd import _lib
    _lib.set_path(request.param)
    yield request.param
    _lib.set_path("auto")


def _expected_tag(route, nz, m, e):
    return TAG_DENSE_WAVE if (route == "auto" and _in_wave_family(nz, m, e)) else TAG_DENSE_GENERIC


# ------------------------------------------------------------------ inputs and the oracle's answers (computed once, shared)
def _seed(nz, m, e):
    return 1000 * nz + 10 * m + e


@functools.lru_cache(maxsize=None)
def _inputs(nz, m, e, nb=B):
    from lcp_physics_amd import scenes
    lcp = scenes.make_random_lcp(nb, nz, m, e, seed=_seed(nz, m, e), dtype=torch.float64)
    cot = torch.randn(nb, nz, generator=torch.Generator().manual_seed(_seed(nz, m, e) + 1), dtype=torch.float64)
    return lcp, cot


@functools.lru_cache(maxsize=None)
def _oracle(nz, m, e, max_iter):
    lcp, cot = _inputs(nz, m, e)
    ref = O.lcp_forward(*lcp, max_iter=max_iter)
    gref = O.lcp_backward(ref, *lcp, cot)
    return ref, {k: gref["d" + k] for k in GRAD_KEYS}


# ------------------------------------------------------------------ the kernels
def _tag(ws):
    return int(ws[-256:-252].cpu().numpy().view(np.int32)[0])


def _run(lcp, cot, max_iter=10):
    """Forward and backward through the fp64 entry points; everything back on the host."""
    from lcp_physics_amd.lcp import lcp_backward, lcp_solve
    sol = lcp_solve(*[None if t is None else t.to(DEV).contiguous() for t in lcp], max_iter=max_iter)
    grads = lcp_backward(sol, cot.to(DEV))
    torch.cuda.synchronize()
    assert sol.x.dtype == torch.float64 and all(g is None or g.dtype == torch.float64 for g in grads)
    out = {k: (None if getattr(sol, k) is None else getattr(sol, k).cpu()) for k in ("x", "y", "z", "s", "iters", "status")}
    out["tag"] = _tag(sol.ws)
    out["grads"] = {k: (None if g is None else g.cpu()) for k, g in zip(GRAD_KEYS, grads)}
    return out


def _check_against_oracle(got, ref, gref, e, what):
    """The gates of this module, no mask: returns the measured maxima (forward, gradients)."""
    fwd = {k: float(parity.rel_err(got[k], getattr(ref, k)).max()) for k in ("x", "z", "s")}
    if e > 0:
        fwd["y"] = float(parity.rel_err(got["y"], ref.y).max())
    else:
        assert got["y"] is None and ref.y is None, what
    grd = {}
    for k in GRAD_KEYS:
        if gref[k] is None:
            assert got["grads"][k] is None, (what, "d" + k, "the oracle has none")
            continue
        assert got["grads"][k] is not None, (what, "d" + k, "missing")
        assert bool(torch.isfinite(got["grads"][k]).all()), (what, "d" + k, "not finite")
        grd[k] = float(parity.rel_err(got["grads"][k], gref[k]).max())
    print("dense_f64 %s  fwd %s  grad %s" % (what, " ".join("%s=%.2e" % kv for kv in fwd.items()),
                                            " ".join("d%s=%.2e" % kv for kv in grd.items())))
    assert max(fwd.values()) < TOL_X64, (what, fwd)
    assert torch.equal(got["iters"].to(torch.int64), ref.iters.to(torch.int64)), (what, "iterations", got["iters"].tolist(), ref.iters.tolist())
    assert int(got["status"].abs().max()) == 0, (what, "status", got["status"].tolist())
    assert max(grd.values()) < TOL_G64, (what, grd)
    return fwd, grd


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _assert_same_bits(a, b, what):
    """Scene-wise outputs `a` and `b` of `_run` (same shapes): every forward output and every gradient bit for bit."""
    for k in ("x", "y", "z", "s", "iters", "status"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, torch.nonzero(_bits(a[k]) != _bits(b[k]))[:4].tolist())
    for k in GRAD_KEYS:
        ga, gb = a["grads"][k], b["grads"][k]
        assert (ga is None) == (gb is None), (what, "d" + k)
        if ga is not None:
            assert torch.equal(_bits(ga), _bits(gb)), (what, "d" + k, torch.nonzero(_bits(ga) != _bits(gb))[:4].tolist())


def _scenes_of(out, idx):
    """Rows `idx` of a batched result of `_run`."""
    sub = {k: (None if out[k] is None else out[k][idx]) for k in ("x", "y", "z", "s", "iters", "status")}
    sub["grads"] = {k: (None if g is None else g[idx]) for k, g in out["grads"].items()}
    return sub


def _take(lcp, idx):
    return tuple(None if t is None else t[idx] for t in lcp)


# ------------------------------------------------------------------ host only: what makes the unmasked gates legitimate
def _permuted(lcp, cot, seed):
    Q, p, G, h, A, b, F = lcp
    nz, m = Q.shape[1], G.shape[1]
    g = torch.Generator().manual_seed(seed)
    px, pm = torch.randperm(nz, generator=g), torch.randperm(m, generator=g)
    if A is None:
        Ap, bp, pe = None, None, None
    else:
        pe = torch.randperm(A.shape[1], generator=g)
        Ap, bp = A[:, pe][:, :, px], b[:, pe]
    args = (Q[:, px][:, :, px], p[:, px], G[:, pm][:, :, px], h[:, pm], Ap, bp, F[:, pm][:, :, pm])
    inv = lambda q: None if q is None else torch.argsort(q)
    return args, cot[:, px], inv(px), inv(pm), inv(pe)


@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_oracle_agrees_with_itself_under_reordering(shape, max_iter):
    """The oracle alone, fp64: each LCP solved again with its unknowns, inequality and equality rows randomly permuted (identical
    in exact arithmetic, another elimination order in floating point) gives the same solution, the same seven gradients and
    the same iteration counts.  Nothing on these inputs is decided by rounding - the condition for comparing without a mask."""
    nz, m, e = shape
    lcp, cot = _inputs(nz, m, e)
    ref, gref = _oracle(nz, m, e, max_iter)
    args, cotp, ix, im, ie = _permuted(lcp, cot, seed=_seed(nz, m, e) + 2)
    rp = O.lcp_forward(*args, max_iter=max_iter)
    gp = O.lcp_backward(rp, *args, cotp)
    assert torch.equal(rp.iters, ref.iters), (shape, rp.iters.tolist(), ref.iters.tolist())
    back = {"x": rp.x[:, ix], "z": rp.z[:, im], "s": rp.s[:, im], "Q": gp["dQ"][:, ix][:, :, ix], "p": gp["dp"][:, ix],
            "G": gp["dG"][:, im][:, :, ix], "h": gp["dh"][:, im], "F": gp["dF"][:, im][:, :, im]}
    want = {"x": ref.x, "z": ref.z, "s": ref.s, "Q": gref["Q"], "p": gref["p"], "G": gref["G"], "h": gref["h"], "F": gref["F"]}
    if e > 0:
        back.update({"y": rp.y[:, ie], "A": gp["dA"][:, ie][:, :, ix], "b": gp["db"][:, ie]})
        want.update({"y": ref.y, "A": gref["A"], "b": gref["b"]})
    else:
        assert gp["dA"] is None and gp["db"] is None and gref["A"] is None and gref["b"] is None
    moved = {k: float(parity.rel_err(back[k], want[k]).max()) for k in want}
    assert max(moved.values()) < TOL_SELF, (shape, max_iter, moved)


def test_generic_plan_levels_of_the_shapes():
    """Host only: the three plan-level shapes get the level their comment says.  At these sizes no other kernel family claims a
    larger block, so the per-scene workspace stride that `lcp_workspace_bytes` reports is the layout of lcp_generic.hip's
    `ws_elems` at the level `make_plan` chose (R, Q^-1, GA, S11^-1, x, s, z, y, one count; from level 0 on T and the prefactor
    scratch; at level 2 Q, Q^-1 and G as well)."""
    from lcp_physics_amd import _lib

    def ws_bytes(nz, m, e, level):
        n = m * m + nz * nz + m * e + e * e + nz + 2 * m + e
        if level != 1:
            n += m * (m | 1) + m * nz
        if level == 2:
            n += 2 * nz * nz + m * nz
        return ((n + 1 + 31) & ~31) * 8

    word = _lib.COMPUTE_F64 | _lib.IO_F64 | _lib.PATH_GENERIC
    for (nz, m, e), level in PLAN_LEVEL.items():
        stride = _lib.workspace_bytes(2, nz, m, e, word) - _lib.workspace_bytes(1, nz, m, e, word)
        sizes = {lv: ws_bytes(nz, m, e, lv) for lv in (1, 0, 2)}
        assert len(set(sizes.values())) == 3 and stride == sizes[level], ((nz, m, e), level, stride, sizes)
    assert sorted(PLAN_LEVEL.values()) == [0, 1, 2] and all(s in SHAPES and not _in_wave_family(*s) for s in PLAN_LEVEL)


# ------------------------------------------------------------------ 1. forward and all seven gradients at the family edges
@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", MAX_ITERS)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_forward_and_seven_gradients_match_oracle(shape, max_iter, route):
    nz, m, e = shape
    lcp, cot = _inputs(nz, m, e)
    ref, gref = _oracle(nz, m, e, max_iter)
    got = _run(lcp, cot, max_iter)
    assert got["tag"] == _expected_tag(route, nz, m, e), (shape, route, "workspace tag", got["tag"])
    _check_against_oracle(got, ref, gref, e, "%s %s max_iter=%d tag=%d" % (_id(shape), route, max_iter, got["tag"]))


# ------------------------------------------------------------------ 2. partial hardware units and batch position
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 32, 3), (17, 64, 3)], ids=_id)
def test_scene_in_a_batch_is_bitwise_the_scene_alone(shape, route):
    """Scene k of a batch of 1, 3, 5 or 67 scenes (partial workgroups, partial four-scene units, more than one block) is bit for
    bit scene k solved alone: forward outputs and all seven gradients."""
    nz, m, e = shape
    lcp, cot = _inputs(nz, m, e, 67)
    alone = [_run(_take(lcp, slice(k, k + 1)), cot[k:k + 1]) for k in range(67)]
    for out in alone:
        assert out["tag"] == _expected_tag(route, nz, m, e)
    for nb in (1, 3, 5, 67):
        batch = _run(_take(lcp, slice(0, nb)), cot[:nb])
        assert batch["tag"] == _expected_tag(route, nz, m, e)
        for k in range(nb):
            _assert_same_bits(_scenes_of(batch, slice(k, k + 1)), alone[k], (shape, route, "B=%d" % nb, "scene %d" % k))


# ------------------------------------------------------------------ 3. mixed batches
MIXED = (15, 64, 3)
# which kind sits where: runs of one, two and three of a kind, so that the four scenes of a four-scenes-per-wave unit are of
# every mixture (S = contact-structured, U = unstructured)
MIXED_PATTERN = "SUUSSSUSUUUSUSSU"


@functools.lru_cache(maxsize=None)
def _stack_lcp():
    from lcp_physics_amd import scenes
    sc = scenes.make_stack_scenes(B=B, nbox=4, pts_per_interface=4, seed=1238, dtype=torch.float64)
    lcp = tuple(t.double().contiguous() for t in O.assemble_lcp(*sc.assembly_args()))
    assert (lcp[0].shape[1], lcp[2].shape[1], lcp[4].shape[1]) == MIXED
    return lcp


@pytest.mark.gpu
def test_mixed_batch_scenes_are_bitwise_those_of_homogeneous_batches(route):
    """One fp64 batch interleaves contact-structured scenes (a four-box stack, 16 contacts) with unstructured ones of the same
    sizes: `lcp_classify_wave` decides per scene, with fp64 loads, which kernel solves it.  Every scene comes out bit for bit as
    in a batch of its own kind, and the unstructured ones pass the oracle gates."""
    nz, m, e = MIXED
    assert MIXED_PATTERN.count("S") == B and MIXED_PATTERN.count("U") == B
    rnd, cot_u = _inputs(nz, m, e)
    stk = _stack_lcp()
    cot_s = torch.randn(B, nz, generator=torch.Generator().manual_seed(77), dtype=torch.float64)
    where = {"S": [i for i, c in enumerate(MIXED_PATTERN) if c == "S"], "U": [i for i, c in enumerate(MIXED_PATTERN) if c == "U"]}
    mixed = [torch.empty((2 * B,) + tuple(t.shape[1:]), dtype=torch.float64) for t in rnd]
    cot = torch.empty(2 * B, nz, dtype=torch.float64)
    for t, ts, tu in zip(mixed, stk, rnd):
        t[where["S"]], t[where["U"]] = ts, tu
    cot[where["S"]], cot[where["U"]] = cot_s, cot_u
    got = _run(mixed, cot)
    own = {"S": _run(stk, cot_s), "U": _run(rnd, cot_u)}
    tag = _expected_tag(route, nz, m, e)
    assert (got["tag"], own["S"]["tag"], own["U"]["tag"]) == (tag, tag, tag)
    for kind in "SU":
        _assert_same_bits(_scenes_of(got, where[kind]), own[kind], (route, "kind " + kind))
    ref, gref = _oracle(nz, m, e, 10)
    _check_against_oracle(_scenes_of(got, where["U"]), ref, gref, e, "%s %s mixed batch, unstructured scenes" % (_id(MIXED), route))


# ------------------------------------------------------------------ 4. LCPFunction itself
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 32, 3), (7, 23, 0)], ids=_id)
def test_lcp_function_gradients_are_the_direct_backward(shape, route):
    """`LCPFunction()(Q, p, G, h, A, b, F)` on fp64 leaves and `.backward()` with a random cotangent: the seven `.grad`s are bit
    for bit what `lcp_backward` returns for the same solve; with `A = b = torch.tensor([])` (the reference's "no equality
    rows") `A.grad` and `b.grad` stay None as lcp.py:59-60 leaves them."""
    from lcp_physics_amd.lcp import LCPFunction
    nz, m, e = shape
    lcp, cot = _inputs(nz, m, e)
    direct = _run(lcp, cot)
    leaves = [None if t is None else t.to(DEV).requires_grad_(True) for t in lcp]
    if e == 0:
        leaves[4] = torch.tensor([], dtype=torch.float64, requires_grad=True)
        leaves[5] = torch.tensor([], dtype=torch.float64, requires_grad=True)
    fn = LCPFunction()
    x = fn(*leaves)
    x.backward(cot.to(DEV))
    torch.cuda.synchronize()
    assert x.dtype == torch.float64 and torch.equal(_bits(x.detach().cpu()), _bits(direct["x"]))
    assert torch.equal(_bits(fn.lams.cpu()), _bits(direct["z"])) and torch.equal(_bits(fn.slacks.cpu()), _bits(direct["s"]))
    assert _tag(fn.solution.ws) == direct["tag"] == _expected_tag(route, nz, m, e)
    for k, leaf in zip(GRAD_KEYS, leaves):
        want = direct["grads"][k]
        if want is None:
            assert k in "Ab" and e == 0 and leaf.grad is None, (shape, "d" + k)
            continue
        assert leaf.grad is not None and leaf.grad.dtype == torch.float64 and leaf.grad.shape == leaf.shape, (shape, "d" + k)
        assert torch.equal(_bits(leaf.grad.cpu()), _bits(want)), (shape, route, "d" + k)
    if e > 0:
        assert torch.equal(_bits(fn.nus.cpu()), _bits(direct["y"]))
    else:
        assert fn.nus is None and fn.neq == 0
