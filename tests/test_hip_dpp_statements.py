"""The hand-scheduled v_fmac_f64_dpp statements of the sized pinned forward - lu_step_x (LCP_Q_LU_AHEAD, lcp_quad_prims.h) and the
lane masks formed per solve (LCP_Q_MASK_LOCAL).

A step of the LU is one inline-asm statement that updates column K+1, broadcasts the next pivot from it two issue slots later, and spreads
v_rcp_f64 and its Newton steps over the remaining column updates.  The compiler's hazard recogniser does not see inside it: a DPP read
that comes too early, or a read of the reciprocal in the slot behind v_rcp_f64, returns the register's previous contents - a wrong
multiply-add, which shows in exactly these comparisons (tools/isa_lint.py --dpp-all is the static side).  The statements differ per
number of remaining columns, so every sized stack is run (nz 6, 9, 12, 15: 2 to 11 pivots behind the first), at B = 6 - one full
wavefront and one half filled with shadow rows:

  * against the fp64 oracle, with the tolerances of tests/test_hip_form_blocks.py (err_x <= 1e-4, iteration counts equal on the
    16-contact stack and within one elsewhere);
  * bit for bit against the same scenes in a batch of eight (no shadow rows), in a wavefront that mixes topologies against batches of
    one topology each, and beside scenes whose last contact group is dead.
"""
import pytest
import torch

from tests.test_hip_form_blocks import (IT_DELTA, _check_forward, _clone_contacts, _fused, _interleave, _join_last_group, _oracle, _same,
                                        _stack)

pytestmark = pytest.mark.gpu
B = 6


@pytest.mark.parametrize("nbox", [1, 2, 3, 4])
def test_sized_stacks_with_a_half_filled_wavefront(nbox):
    eight = _stack(8, nbox, seed=577)
    sc = eight.slice(0, B)
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, IT_DELTA[nbox])
    _same(out, _fused(eight), list(range(B)), list(range(B)))                   # the shadow rows of the second wave change nothing


def _topologies():
    """stack, joined last group, interleaved list, stack | joined, stack: four topologies in the full wave, two in the half-filled one"""
    sc = _clone_contacts(_stack(B, 4, seed=577))
    _join_last_group(sc, [1, 4])
    _interleave(sc, [2])
    return sc


def test_topologies_mixed_inside_a_wavefront():
    sc = _topologies()
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    plain = _fused(_stack(B, 4, seed=577))
    joined = _clone_contacts(_stack(B, 4, seed=577))
    _join_last_group(joined, range(B))
    inter = _clone_contacts(_stack(B, 4, seed=577))
    _interleave(inter, range(B))
    _same(out, plain, [0, 3, 5], [0, 3, 5])
    _same(out, _fused(joined), [1, 4], [1, 4])
    _same(out, _fused(inter), [2], [2])


def _dead_last_group(sc, scenes_):
    """contacts 12 .. 15 with a zero normal: their rows of Jc and Jt are exact zeros, the last group adds nothing to any block"""
    sc = _clone_contacts(sc)
    for s in scenes_:
        sc.c_n[s, 12:16] = 0.0
    return sc


def test_a_scene_whose_last_contact_group_is_dead():
    sc = _dead_last_group(_stack(B, 4, seed=577), [1, 4])
    G = _oracle(sc)[2][2]
    assert bool((G[[1, 4], 12:16] == 0).all()) and bool((G[[1, 4], 40:48] == 0).all()) and bool((G[[0, 2, 3, 5], 12:16] != 0).any())
    out = _fused(sc)
    ref_v, ref_it, _, _ = _oracle(sc)
    _check_forward(out["v_new"], out["iters"], out["status"], sc, ref_v, ref_it, 1)
    _same(out, _fused(_stack(B, 4, seed=577)), [0, 2, 3, 5], [0, 2, 3, 5])
    _same(out, _fused(_dead_last_group(_stack(B, 4, seed=577), range(B))), [1, 4], [1, 4])
