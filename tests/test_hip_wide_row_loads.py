"""Row loads and row staging of the four-scenes-per-wave kernels (lcp_fwd_quad / lcp_bwd_quad, lcp_quad_kernels.inc) at the edges where
a 16-byte access can go wrong.

Every lane of these kernels fetches its own row of G, A (dense backward, dense forward) or Je (contact-list forward) - nz fp32 entries
at a base that is only dword aligned - and parks it in LDS as 16-byte stores.  The source asks for the entries one by one (row16); for a
compile-time nz the compiler currently merges them into 16-byte loads and a remainder (nz = 15: three dwordx4 and one dwordx3).  Nothing
here pins that choice; what is checked holds for either form: no entry past nz - 1 of a row is read, no alignment beyond a dword is
assumed, every scene gets its own rows.  Forward plus dense backward, on the smallest shapes that reach every unit:

  * stacks of 1 to 4 boxes (nz 6, 9, 12, 15: the four sized units) with 1 and 4 points per interface, one shape with two equality rows
    (the run-time-size kernels) and one call through the dense boundary (LCPFunction);
  * batches of 1, 3 and 5 scenes, so that the last wavefront is partly filled;
  * every scene's outputs in the batch are BIT FOR BIT those of the same scene run alone;
  * the same with G, A and Je carved from a guarded arena (tests/guarded_buffers.py: each buffer is followed by 0xFF bytes - NaN as
    fp32 - so a load past the last row's entry nz - 1 poisons a result; guards intact), and with G as a view one float into its
    allocation (a base that is dword aligned and no more);
  * forward and gradients against the fp64 oracle within the tolerance tests/parity.py states (headline_report: 1e-4)."""
from dataclasses import replace

import pytest
import torch

from oracle import pdipm_oracle as O
from tests import parity
from tests.guarded_buffers import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCHES = (1, 3, 5)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    """Bitwise equality of two result dicts (NaN payloads included); returns the names that differ."""
    bad = []
    for k in a:
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not torch.equal(_bits(a[k]), _bits(b[k]))):
            bad.append(k)
    return bad


def _scenes(B, nbox, pts, rows):
    from lcp_physics_amd import scenes
    sc = scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=pts, seed=77 + 10 * nbox + pts, dtype=torch.float32)
    if rows == 2:                                        # two equality rows: no sized unit (they are built for three) -> run-time sizes
        sc = replace(sc, Je=sc.Je[:, :2].contiguous())
    return sc


def _cot(B, nz):
    return torch.randn(B, nz, generator=torch.Generator().manual_seed(4321), dtype=torch.float32)


def _run(scg, cot, G=None, A=None):
    """Contact-list forward on the four-scenes-per-wave kernels, then the dense backward reading rows of G and A."""
    from lcp_physics_amd.lcp import lcp_backward
    from lcp_physics_amd.physics import assemble_contacts, fused_step
    from lcp_physics_amd.physics.batched_world import solution_of_step
    lcp = assemble_contacts(scg)
    G = lcp[2] if G is None else G
    A = lcp[4] if A is None else A
    out = fused_step(scg, path="quad")
    grads = lcp_backward(solution_of_step(scg, out, G, A), cot.to(DEV))
    torch.cuda.synchronize()
    res = {k: out[k] for k in ("v_new", "z", "s", "y", "iters", "status")}
    res.update({"d" + k: g for k, g in zip("QpGhAbF", grads)})
    return res, lcp


def _row(res, i):
    return {k: (None if v is None else v[i:i + 1]) for k, v in res.items()}


def _check_oracle(res, lcp, cot):
    """Forward and gradients against the fp64 oracle (tests/parity.py::headline_report and the tolerance it states); returns the
    number of scenes whose backward system is well posed - the gradient figures exist only where there is one."""
    B = cot.shape[0]
    lcp64 = [None if t is None else t.double().cpu() for t in lcp]
    grads = {k: (None if res["d" + k] is None else res["d" + k].cpu()) for k in "QpGhAbF"}
    rep, _ = parity.headline_report(O, lcp64, -res["v_new"].reshape(B, -1).cpu(), res["z"].cpu(), res["s"].cpu(), res["iters"].cpu(),
                                    cot=cot, grads=grads)
    tol = rep["tolerance"]
    shown = {k: rep[k] for k in ("fwd_err_x_max", "bwd_well_posed_scenes", "bwd_err_dp_max", "bwd_err_dQ_max", "bwd_err_dA_max",
                                 "bwd_err_db_max") if k in rep}
    print("oracle parity:", shown)
    assert rep["fwd_err_x_max"] <= tol, shown
    assert rep["bwd_nonfinite_scenes"] == 0, rep
    if rep["bwd_well_posed_scenes"] > 0:
        for k in ("bwd_err_dp_max", "bwd_err_dQ_max", "bwd_err_dA_max", "bwd_err_db_max"):
            assert rep[k] <= tol, shown
    return rep["bwd_well_posed_scenes"]


def _case(nbox, pts, rows=3):
    well_posed = 0
    for B in BATCHES:
        sc = _scenes(B, nbox, pts, rows)
        scg = sc.to(device=DEV)
        cot = _cot(B, 3 * sc.nb)
        res, lcp = _run(scg, cot)
        # (1) every scene of the batch against the same scene run alone
        for i in range(B):
            alone, _ = _run(sc.slice(i, i + 1).to(device=DEV), cot[i:i + 1])
            assert _same(_row(res, i), alone) == [], "B=%d scene %d differs from the scene run alone" % (B, i)
        # (2) G, A, Je end their allocations' payload right in front of NaN bytes
        ar = Arena(B, DEV)
        ar.add("G", torch.float32, lcp[2].shape, data=lcp[2]).add("A", torch.float32, lcp[4].shape, data=lcp[4])
        ar.add("Je", torch.float32, scg.Je.shape, data=scg.Je)
        ar.build()
        snap = ar.snapshot_inputs()
        guarded, _ = _run(replace(scg, Je=ar["Je"]), cot, G=ar["G"], A=ar["A"])
        assert _same(res, guarded) == [], "B=%d: results change when the rows end in front of NaN bytes" % B
        assert ar.check() == [] and ar.inputs_unchanged(snap) == []
        # (3) G at a base that is dword aligned and no more
        flat = torch.full((lcp[2].numel() + 1,), float("nan"), dtype=torch.float32, device=DEV)
        Goff = flat[1:].view(lcp[2].shape)
        Goff.copy_(lcp[2])
        assert Goff.data_ptr() % 16 == 4 and Goff.is_contiguous()
        shifted, _ = _run(scg, cot, G=Goff)
        assert _same(res, shifted) == [], "B=%d: results change with G one float into its allocation" % B
        # (4) the fp64 oracle
        well_posed += _check_oracle(res, lcp, cot)
    assert well_posed >= 1, "no scene of the three batches has a well-posed backward: the gradients were compared nowhere"


@pytest.mark.parametrize("pts", [1, 4])
@pytest.mark.parametrize("nbox", [1, 2, 3, 4])
def test_sized_units(nbox, pts):
    """nz = 3 (nbox + 1) = 6, 9, 12, 15 with three pinned equality rows: lcp_quad_n{6,9,12,15}e3; one point per interface leaves the
    contact count off the shape's own (the run-time-count instantiations of the same units)."""
    _case(nbox, pts)


def test_run_time_sizes():
    """Two equality rows: no sized unit serves them, the run-time-size kernels of lcp_quad.hip do."""
    _case(3, 4, rows=2)


def test_dense_boundary():
    """LCPFunction on the assembled (Q, p, G, h, A, b, F): the dense forward's loader (load_dense_q) reads the rows of G and A, the dense
    backward follows through autograd.  The same four checks: batch against single scenes, G and A in front of NaN bytes, G one float
    into its allocation, forward and gradients against the fp64 oracle."""
    from lcp_physics_amd.lcp import LCPFunction
    from lcp_physics_amd.physics import assemble_contacts

    def solve(lcp, cot):
        ins = [None if t is None else t.detach().requires_grad_(True) for t in lcp]      # (detach, not clone: the kernels must read THESE buffers)
        assert all(t is None or i.data_ptr() == t.data_ptr() for i, t in zip(ins, lcp))
        x = LCPFunction(path="quad")(*ins)
        x.backward(cot.to(DEV))
        torch.cuda.synchronize()
        res = {"x": x.detach()}
        res.update({"d" + k: (None if t is None else t.grad) for k, t in zip("QpGhAbF", ins)})
        return res

    def oracle(res, lcp, cot):
        """As _check_oracle; LCPFunction returns x only, so the multipliers the report's index-set fields read are the oracle's own."""
        B = cot.shape[0]
        lcp64 = [None if t is None else t.double().cpu() for t in lcp]
        ref = O.lcp_forward(*lcp64)
        grads = {k: (None if res["d" + k] is None else res["d" + k].cpu()) for k in "QpGhAbF"}
        rep, _ = parity.headline_report(O, lcp64, res["x"].cpu(), ref.z, ref.s, ref.iters, cot=cot, grads=grads, cache={"ref": ref})
        shown = {k: rep[k] for k in ("fwd_err_x_max", "bwd_well_posed_scenes", "bwd_err_dp_max", "bwd_err_dQ_max", "bwd_err_dA_max",
                                     "bwd_err_db_max") if k in rep}
        print("dense boundary B=%d oracle parity:" % B, shown)
        assert rep["fwd_err_x_max"] <= rep["tolerance"], shown
        assert rep["bwd_nonfinite_scenes"] == 0, rep
        if rep["bwd_well_posed_scenes"] > 0:
            for k in ("bwd_err_dp_max", "bwd_err_dQ_max", "bwd_err_dA_max", "bwd_err_db_max"):
                assert rep[k] <= rep["tolerance"], shown
        return rep["bwd_well_posed_scenes"]

    well_posed = 0

    for B in BATCHES:
        sc = _scenes(B, 4, 4, 3)
        lcp = assemble_contacts(sc.to(device=DEV))
        cot = _cot(B, 3 * sc.nb)
        res = solve(lcp, cot)
        for i in range(B):
            alone = solve([None if t is None else t[i:i + 1].contiguous() for t in lcp], cot[i:i + 1])
            assert _same(_row(res, i), alone) == [], "B=%d scene %d differs from the scene run alone" % (B, i)
        ar = Arena(B, DEV)
        ar.add("G", torch.float32, lcp[2].shape, data=lcp[2]).add("A", torch.float32, lcp[4].shape, data=lcp[4])
        ar.build()
        guarded = solve([ar["G"] if k == 2 else (ar["A"] if k == 4 else t) for k, t in enumerate(lcp)], cot)
        assert _same(res, guarded) == [], "B=%d: results change when the rows end in front of NaN bytes" % B
        assert ar.check() == []
        flat = torch.full((lcp[2].numel() + 1,), float("nan"), dtype=torch.float32, device=DEV)
        Goff = flat[1:].view(lcp[2].shape)
        Goff.copy_(lcp[2])
        assert Goff.data_ptr() % 16 == 4 and Goff.is_contiguous()
        shifted = solve([Goff if k == 2 else t for k, t in enumerate(lcp)], cot)
        assert _same(res, shifted) == [], "B=%d: results change with G one float into its allocation" % B
        well_posed += oracle(res, lcp, cot)
    assert well_posed >= 1, "no scene of the three batches has a well-posed backward: the gradients were compared nowhere"
