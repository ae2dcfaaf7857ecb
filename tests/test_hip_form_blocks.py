"""The formation of K = Q + G^T M^-1 G by (group of four contacts, body block) - LCP_Q_FORM_BLOCKS in lcp_quad_kernels.inc.

The size-specialised pinned forward with register columns (`lcp_fwd_quad<..., ALG = 2, NZF, EF, ..., COLR>`: the fused step, the dense
boundary and the run-time-count form, while a wavefront has its SIMD to itself) reads one wave-uniform mask - which of the 4 x 4
(group, block) pairs hold anything but exact zeros in ANY of the wave's four scenes - and skips the others.  What can go wrong is the
mask (a block left out that a scene of the wave needs) and the wave-uniform branch (a scene's result depending on its neighbours), so:

  * the plain stack at every sized shape (one to four boxes, four points per interface; one box has a single free block);
  * one wavefront whose four scenes differ in topology - the stack, a scene whose last group joins box 1 and box 4, a scene whose
    contact list is interleaved so that every group meets every body pair (all bits set) - against the fp64 oracle AND bit for bit
    against batches of one topology (the repository's rule for wave-uniform branches);
  * per-scene contact counts that leave the last one or two groups dead - beside full lists, in the wavefront of four different scenes, and
    in wavefronts where every scene does (bits cleared by dead lanes alone); a batch whose group 0 is dead (zero rows) and later groups live;
  * the same through the dense LCPFunction boundary (masks from rows of G), the dense backward behind either forward and
    lcp_step_backward_f32, whose one formation per launch takes the block form too (LCP_Q_FORM_BLOCKS_BWD).

Tolerances: tests/test_hip_headline_parity.py's - err_x <= 1e-4 on new_v, iteration counts equal on the 16-contact stack (STRICT) and
within one where the solves converge to rounding or the topology is rewritten (CONVERGED), gradients <= 1e-4.  8 to 32 scenes, path
"quad" (four scenes per wavefront at every batch size).
"""
import pytest
import torch

from oracle import pdipm_oracle as O
from tests import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
# iteration counts against the oracle's, with the gates of tests/test_hip_headline_parity.py: equal on the 16-contact stack (STRICT), within
# one on the smaller stacks, whose solves converge to rounding inside the ten iterations so that the exit tests of pdipm.py:133 compare
# rounding noise (CONVERGED)
IT_DELTA = {1: 1, 2: 1, 3: 1, 4: 0}
CONTACT_FIELDS = ("c_n", "c_p1", "c_p2", "c_i1", "c_i2")


def _stack(B, nbox, seed=311):
    from lcp_physics_amd import scenes
    return scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=4, seed=seed, dtype=torch.float32)


def _clone_contacts(sc):
    for k in CONTACT_FIELDS:
        setattr(sc, k, getattr(sc, k).clone())
    return sc


def _join_last_group(sc, scenes_):
    """contacts 12 .. 15 (box 3 - box 4 on the stack) become contacts between box 1 and box 4: blocks 0 and 3 for the last group"""
    for s in scenes_:
        sc.c_p1[s, 12:16] += (sc.p[s, 3, 1:] - sc.p[s, 1, 1:]).to(sc.c_p1.dtype)     # the same world points, seen from box 1's centre
        sc.c_i1[s, 12:16] = 1
        sc.c_i2[s, 12:16] = 4


def _interleave(sc, scenes_):
    """contact 4 g + k <- contact 4 k + g: every group of four holds one contact of every interface, every mask bit is set"""
    perm = torch.tensor([4 * (c % 4) + c // 4 for c in range(16)])
    for s in scenes_:
        for k in CONTACT_FIELDS:
            t = getattr(sc, k)
            t[s] = t[s][perm]


def _mixed(B=8):
    """per wavefront: stack, joined last group, interleaved list, stack"""
    sc = _clone_contacts(_stack(B, 4))
    _join_last_group(sc, range(1, B, 4))
    _interleave(sc, range(2, B, 4))
    return sc


def _oracle(sc, counts=None):
    """fp64 oracle on the fp32 LCP the scenes assemble to (as tests/test_hip_headline_parity.py); `counts`: per-scene live contacts (the oracle gets each scene's truncated list)"""
    if counts is None:
        from lcp_physics_amd.physics import assemble_contacts
        lcp = [None if t is None else t.double().cpu() for t in assemble_contacts(sc.to(device=DEV))]   # identical inputs: the fp32 LCP
        sol = O.lcp_forward(*lcp)
        return -sol.x, sol.iters, lcp, sol
    xs, its = [], []
    for s, c in enumerate(counts):
        one = sc.slice(s, s + 1)
        for k in CONTACT_FIELDS:
            setattr(one, k, getattr(one, k)[:, :c])
        v, it, _, _ = _oracle(one)
        xs.append(v)
        its.append(it)
    return torch.cat(xs), torch.cat(its), None, None


def _check_forward(v_new, iters, status, sc, ref_v, ref_it, it_delta):
    assert int((status.cpu() & ~4 != 0).sum()) == 0, status
    Q = torch.diag_embed(sc.Mdiag.reshape(sc.B, -1).double())
    p = (sc.Mdiag * sc.v + sc.dt * sc.f).reshape(sc.B, -1).double()
    ex = parity.err_x(-v_new.reshape(sc.B, -1).double().cpu(), -ref_v, Q, p)
    d = (iters.cpu().int() - ref_it.int()).abs()
    print("err_x max %.3g, iteration delta max %d" % (float(ex.max()), int(d.max())))
    assert float(ex.max()) <= 1e-4, ex
    assert int(d.max()) <= it_delta, d


def _fused(sc):
    from lcp_physics_amd.physics import fused_step
    out = fused_step(sc.to(device=DEV), path="quad")
    torch.cuda.synchronize()
    return out


def _same(a, b, idx_a, idx_b, keys=("v_new", "z", "s", "iters", "status")):
    for k in keys:
        assert torch.equal(a[k][idx_a], b[k][idx_b]), k


@pytest.mark.parametrize("nbox", [1, 2, 3, 4])
def test_plain_stack_at_every_sized_shape(nbox):
    sc = _stack(32, nbox)
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, IT_DELTA[nbox])


def test_one_wavefront_of_four_topologies_and_no_dependence_on_neighbours():
    B = 8
    sc = _mixed(B)
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    plain = _fused(_stack(B, 4))
    inter = _clone_contacts(_stack(B, 4))
    _interleave(inter, range(B))
    inter = _fused(inter)
    _same(out, plain, [0, 3, 4, 7], [0, 3, 4, 7])
    _same(out, inter, [2, 6], [2, 6])


def test_stack_and_joined_scenes_share_wavefronts_by_blocks():
    """Without an interleaved scene the wave's mask is the stack's seven bits and the joined group's block 0: a union that is neither
    scene's own mask.  The joined scenes must return what they return in the waves of `_mixed`, whose masks are full."""
    B = 8
    sc = _clone_contacts(_stack(B, 4))
    _join_last_group(sc, range(1, B, 2))
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    _same(out, _fused(_stack(B, 4)), [0, 2, 4, 6], [0, 2, 4, 6])
    mixed = _fused(_mixed(B))
    _same(out, mixed, [1, 5], [1, 5])


def _count_entry(sc, cnt):
    """lcp_solve_dynamics_f32 with per-scene contact counts: the run-time-count instantiation a ContactWorld gets"""
    from lcp_physics_amd.physics.batched_world import rows_pin_leading_coordinates, solve_dynamics
    from lcp_physics_amd.physics.contacts import ContactBuffers
    scg = sc.to(device=DEV)
    cb = ContactBuffers(sc.B, sc.nb, sc.nc, DEV)
    cb.c_n, cb.c_p1, cb.c_p2, cb.c_i1, cb.c_i2 = scg.c_n, scg.c_p1, scg.c_p2, scg.c_i1, scg.c_i2
    out = solve_dynamics(sc.B, sc.nb, sc.nc, 3, torch.tensor(cnt, dtype=torch.int32, device=DEV), scg.Mdiag, scg.v, scg.f, scg.rest,
                         scg.fric, cb, scg.Je, sc.dt, path="quad", pinned=rows_pin_leading_coordinates(scg.Je))
    torch.cuda.synchronize()
    return out


def test_four_different_scenes_in_a_wavefront_with_per_scene_counts():
    """stack, joined last group, interleaved list, and a stack whose count leaves the last one or two groups dead: one wavefront"""
    B = 8
    sc = _mixed(B)
    counts = [16, 16, 16, 12, 16, 16, 16, 8]
    out = _count_entry(sc, counts)
    ref_v, ref_it, _, _ = _oracle(sc, counts)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    plain = _count_entry(_stack(B, 4), counts)
    inter = _clone_contacts(_stack(B, 4))
    _interleave(inter, range(B))
    inter = _count_entry(inter, [16] * B)
    _same(out, plain, [0, 3, 4, 7], [0, 3, 4, 7], keys=("v_new", "iters", "status"))
    _same(out, inter, [2, 6], [2, 6], keys=("v_new", "iters", "status"))


def test_wavefronts_whose_scenes_all_leave_the_last_groups_dead():
    """Counts 8, 8, 12, 8 and 4, 8, 8, 8: the union over the wave clears the bits of group 3 / groups 2 and 3, because dead contact lanes
    hold zero rows.  Besides the oracle: the scenes that keep their count must return bit for bit what they return among neighbours with
    full lists, where the wave's mask is the whole stack's - the skipped blocks added nothing."""
    B = 8
    sc = _stack(B, 4)
    counts = [8, 8, 12, 8, 4, 8, 8, 8]
    out = _count_entry(sc, counts)
    ref_v, ref_it, _, _ = _oracle(sc, counts)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    among_full = _count_entry(sc, [8, 16, 12, 16, 4, 16, 8, 16])
    _same(out, among_full, [0, 2, 4, 6], [0, 2, 4, 6], keys=("v_new", "iters", "status"))


def _dead_group0(sc):
    """contacts 0 .. 3 with a zero normal: their rows of Jc and Jt are exact zeros (the tangent is the normal turned by a quarter), so
    group 0 sets no bit while groups 1 .. 3 are live"""
    sc = _clone_contacts(sc)
    sc.c_n[:, 0:4] = 0.0
    return sc


def test_group_0_entirely_dead_and_later_groups_live():
    B = 8
    sc = _dead_group0(_stack(B, 4))
    lcp = _oracle(sc)[2]
    G = lcp[2]
    assert bool((G[:, 0:4] == 0).all()) and bool((G[:, 16:24] == 0).all()) and bool((G[:, 4:16] != 0).any())      # the case is what it says
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    # half of each wavefront plain stacks: there the wave's mask has group 0's bit, and the dead-group scenes must not notice
    half = _clone_contacts(_stack(B, 4))
    half.c_n[0::2, 0:4] = 0.0
    out2 = _fused(half)
    _same(out, out2, [0, 2, 4, 6], [0, 2, 4, 6])


def test_per_scene_counts_that_leave_the_last_groups_dead():
    B = 8
    sc = _stack(B, 4)
    counts = [16, 12, 16, 8, 8, 16, 12, 16]
    out = _count_entry(sc, counts)
    ref_v, ref_it, _, _ = _oracle(sc, counts)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    full = _count_entry(sc, [16] * B)
    i_full = [s for s, c in enumerate(counts) if c == 16]
    _same(out, full, i_full, i_full, keys=("v_new", "iters", "status"))


def _dense(sc, cot=None):
    from lcp_physics_amd.lcp import lcp_backward, lcp_solve
    from lcp_physics_amd.physics import assemble_contacts
    lcp = assemble_contacts(sc.to(device=DEV))
    sol = lcp_solve(*lcp, path="quad")
    grads = None if cot is None else lcp_backward(sol, cot.to(DEV))
    torch.cuda.synchronize()
    return lcp, sol, grads


@pytest.mark.parametrize("case", ["stack1", "stack2", "stack3", "stack4", "mixed"])
def test_dense_boundary_masks_from_rows_of_G(case):
    B = 8
    sc = _mixed(B) if case == "mixed" else _stack(B, int(case[-1]))
    lcp, sol, _ = _dense(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(-sol.x, sol.iters, sol.status, sc, ref_v, ref_it, 1 if case == "mixed" else IT_DELTA[int(case[-1])])
    if case == "mixed":
        _, plain, _ = _dense(_stack(B, 4))
        inter = _clone_contacts(_stack(B, 4))
        _interleave(inter, range(B))
        _, inter, _ = _dense(inter)
        for k in ("x", "z", "s", "iters", "status"):
            assert torch.equal(getattr(sol, k)[[0, 3, 4, 7]], getattr(plain, k)[[0, 3, 4, 7]]), k
            assert torch.equal(getattr(sol, k)[[2, 6]], getattr(inter, k)[[2, 6]]), k


# the gradients tests/test_hip_headline_parity.py::check_gates holds against the oracle, and its tolerances: dl/dp, dQ, dA, db and the
# physical Mdiag, v, f at 1e-4, the backward at the kernel's own iterate at 1e-4, the KKT residual of (dx, dlam, dnu) at 1e-6 on EVERY
# scene.  (dG, dh, dF are not determined with four points per interface - redundant normal multipliers - there as here.)
BWD_ERR_KEYS = ("bwd_err_dp_max", "bwd_err_dQ_max", "bwd_err_dA_max", "bwd_err_db_max", "bwd_err_phys_max", "bwd_own_iterate_err_max")


def _check_backward_report(K):
    from tests.test_hip_headline_parity import report
    rep, _ = report(K, None, input_stability=True)
    print({k: v for k, v in rep.items() if k.startswith("bwd") or k.startswith("fwd") or k == "scenes"})
    assert rep["status_nonzero"] == 0 and rep["fwd_err_x_max"] <= 1e-4, rep
    assert rep["bwd_nonfinite_scenes"] == 0, rep
    assert rep["bwd_kkt_resid_all_max"] <= 1e-6, rep
    assert rep["bwd_own_iterate_determined_scenes"] >= 0.5 * rep["scenes"] and rep["bwd_well_posed_frac"] >= 0.5, rep    # (CONVERGED's floor)
    for k in BWD_ERR_KEYS:
        assert rep[k] <= 1e-4, (k, rep)


def _fused_both_backwards(sc, cot):
    """fused step, then the dense seven of lcp_pdipm_backward_f32 and lcp_step_backward_f32's physical gradients"""
    from lcp_physics_amd.lcp import lcp_backward
    from lcp_physics_amd.physics import assemble_contacts, fused_step
    from lcp_physics_amd.physics.batched_world import fused_step_backward, solution_of_step
    B, nz = sc.B, 3 * sc.nb
    scg = sc.to(device=DEV)
    lcp = assemble_contacts(scg)
    out = fused_step(scg, path="quad")
    phys = fused_step_backward(scg, out, (-cot).reshape(B, sc.nb, 3).to(DEV))
    grads = lcp_backward(solution_of_step(scg, out, lcp[2], lcp[4]), cot.to(DEV))
    torch.cuda.synchronize()
    return {"sc": sc, "scg": scg, "lcp": lcp, "cot": cot, "grads": grads, "phys_grads": phys, "pile": False, "entry": "fused",
            "x": -out["v_new"].reshape(B, nz), "z": out["z"], "s": out["s"], "iters": out["iters"], "status": out["status"], "out": out}


def test_both_backwards_behind_the_fused_step_on_the_mixed_wavefront():
    B = 8
    cot = torch.randn(B, 15, generator=torch.Generator().manual_seed(4321), dtype=torch.float32)
    K = _fused_both_backwards(_mixed(B), cot)
    _check_backward_report(K)
    plain = _fused_both_backwards(_stack(B, 4), cot)
    inter = _clone_contacts(_stack(B, 4))
    _interleave(inter, range(B))
    inter = _fused_both_backwards(inter, cot)
    for other, idx in ((plain, [0, 3, 4, 7]), (inter, [2, 6])):
        for g, go in zip(K["grads"], other["grads"]):
            assert (g is None) == (go is None) and (g is None or torch.equal(g[idx], go[idx]))
        for k, g in K["phys_grads"].items():
            assert torch.equal(g[idx], other["phys_grads"][k][idx]), k


def test_dense_backward_on_the_mixed_wavefront():
    B = 8
    sc = _mixed(B)
    cot = torch.randn(B, 3 * sc.nb, generator=torch.Generator().manual_seed(4321), dtype=torch.float32)
    lcp, sol, grads = _dense(sc, cot)
    K = {"sc": sc, "lcp": lcp, "cot": cot, "grads": grads, "phys_grads": None, "pile": False, "entry": "dense",
         "x": sol.x, "z": sol.z, "s": sol.s, "iters": sol.iters, "status": sol.status}
    _check_backward_report(K)
    _, _, plain = _dense(_stack(B, 4), cot)
    inter = _clone_contacts(_stack(B, 4))
    _interleave(inter, range(B))
    _, _, inter = _dense(inter, cot)
    for other, idx in ((plain, [0, 3, 4, 7]), (inter, [2, 6])):
        for g, go in zip(grads, other):
            assert (g is None) == (go is None) and (g is None or torch.equal(g[idx], go[idx]))
