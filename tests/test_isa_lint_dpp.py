"""The wait-state check of tools/isa_lint.py (`dpp_hazard`, `make lint`'s second line).

The v_fmac_f64_dpp statements of lcp_quad_prims.h are inline asm, which the compiler's hazard recogniser does not see.  gfx950 needs two
issue slots between a VALU write of a VGPR and a read of it through a DPP control (tools/microbench/dpp_hazard.hip: stale reads without
them), and one between a transcendental instruction (v_rcp_f64 ...) and a VALU read of its result.  The statements keep both by
construction; these tests hold the tool to hand-written snippets and the shipped assembly to zero findings.  No GPU needed."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

DPP = "row_newbcast:3 row_mask:0xf bank_mask:0xf"


def _kernel(body):
    return "_Z6kernelv:\n; %bb.0:\n" + "".join("\t%s\n" % l if not l.endswith(":") else l + "\n" for l in body) + "\ts_endpgm\n.Lfunc_end0:\n"


def _finds(body):
    lines = _kernel(body).split("\n")
    out = []
    for name, lo, hi in isa_lint.kernels_of(lines):
        isa_lint.dpp_hazard(lines, name, lo, hi, quiet=out)
    return [(reg, text.split()[0], rule) for _, reg, text, _, rule in out]


def test_a_dpp_read_one_or_two_slots_behind_the_write_is_found():
    fmac = "v_fmac_f64_dpp v[0:1], v[4:5], v[8:9] " + DPP
    hit = [("v4", "v_fmac_f64_dpp", "dpp"), ("v5", "v_fmac_f64_dpp", "dpp")]
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", fmac]) == hit
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_mov_b32 s0, 0", fmac]) == hit              # one slot is not enough
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_nop 0", fmac]) == hit
    # the builtin's two-instruction form, and a 32-bit DPP move
    assert _finds(["v_add_f64 v[4:5], v[2:3], v[2:3]", "v_mov_b64_dpp v[6:7], v[4:5] %s bound_ctrl:1" % DPP]) == \
        [("v4", "v_mov_b64_dpp", "dpp"), ("v5", "v_mov_b64_dpp", "dpp")]
    assert _finds(["v_mov_b32_e32 v4, v2", "v_mov_b32_dpp v6, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"]) == [("v4", "v_mov_b32_dpp", "dpp")]
    # a statement that writes its own DPP source: the chain of the microbenchmark
    assert _finds(["s_nop 1", "v_fmac_f64_dpp v[4:5], v[4:5], v[8:9] " + DPP, "v_fmac_f64_dpp v[0:1], v[4:5], v[8:9] " + DPP]) == hit


def test_a_hazard_across_a_label_counts_the_predecessors_last_slots():
    fmac = "v_fmac_f64_dpp v[0:1], v[4:5], v[8:9] " + DPP
    hit = [("v4", "v_fmac_f64_dpp", "dpp"), ("v5", "v_fmac_f64_dpp", "dpp")]
    # fall-through into a labelled block
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", ".LBB0_1:", fmac]) == hit
    # the write sits in front of a branch: the taken edge carries it (one slot - the branch - between), the long way round does not
    body = ["s_cmp_eq_u32 s0, 0", "v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_cbranch_scc1 .LBB0_2", "; %bb.1:", "s_nop 1", "v_mov_b32_e32 v9, 0",
            ".LBB0_2:", fmac]
    assert _finds(body) == hit
    # a loop's back edge: the write at the bottom reaches the read at the top
    loop = [".LBB0_1:", fmac, "s_nop 1", "s_add_u32 s0, s0, 1", "s_cmp_lt_u32 s0, 4", "v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_cbranch_scc1 .LBB0_1"]
    assert _finds(loop) == hit
    # ... and with two slots on every path into the block nothing is found
    assert _finds(["s_cmp_eq_u32 s0, 0", "v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_nop 0", "s_cbranch_scc1 .LBB0_2", "; %bb.1:", "s_nop 1",
                   ".LBB0_2:", fmac]) == []


def test_covered_reads_are_not_flagged():
    fmac = "v_fmac_f64_dpp v[0:1], v[4:5], v[8:9] " + DPP
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", "s_nop 1", fmac]) == []                        # the blanket rule of the statements
    assert _finds(["v_mul_f64 v[4:5], v[2:3], v[2:3]", "v_mul_f64 v[10:11], v[2:3], v[2:3]", "v_mul_f64 v[12:13], v[2:3], v[2:3]", fmac]) == []
    # lu_step_x: column K+1 written, two column updates, then the next pivot's broadcast reads it
    assert _finds(["s_nop 1", "v_fmac_f64_dpp v[4:5], v[4:5], -v[8:9] " + DPP, "v_fmac_f64_dpp v[12:13], v[12:13], -v[8:9] " + DPP,
                   "v_fmac_f64_dpp v[14:15], v[14:15], -v[8:9] " + DPP, "v_mov_b64_dpp v[6:7], v[4:5] row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1"]) == []
    # loads are not VALU writes (s_waitcnt orders them), and SGPR spills to lanes are read without DPP
    assert _finds(["ds_read_b64 v[4:5], v20", "s_waitcnt lgkmcnt(0)", fmac]) == []
    assert _finds(["v_writelane_b32 v4, s0, 3", "v_readlane_b32 s1, v4, 3"]) == []


def test_a_write_of_the_plain_multiplier_or_the_accumulator_is_no_hazard():
    fmac = "v_fmac_f64_dpp v[0:1], v[4:5], v[8:9] " + DPP
    assert _finds(["v_cvt_f64_f32_e32 v[8:9], v30", fmac]) == []                                     # the multiplier: a plain read
    assert _finds(["v_mov_b64_e32 v[0:1], 0", fmac]) == []                                            # the accumulator
    assert _finds(["v_cndmask_b32_e32 v9, 0, v31, vcc", "v_fmac_f64_dpp v[0:1], v[4:5], -v[8:9] " + DPP]) == []


def test_a_transcendental_result_needs_one_slot_before_a_valu_read():
    hit = [("v4", "v_fma_f64", "trans"), ("v5", "v_fma_f64", "trans")]
    assert _finds(["v_rcp_f64_e32 v[4:5], v[2:3]", "v_fma_f64 v[6:7], -v[2:3], v[4:5], 1.0"]) == hit
    assert _finds(["v_rcp_f64_e32 v[4:5], v[2:3]", "s_nop 0", "v_fma_f64 v[6:7], -v[2:3], v[4:5], 1.0"]) == []
    assert _finds(["v_rcp_f64_e32 v[4:5], v[2:3]", "v_fmac_f64_dpp v[0:1], v[10:11], v[8:9] " + DPP, "v_fma_f64 v[6:7], -v[2:3], v[4:5], 1.0"]) == []
    assert _finds(["v_rcp_f64_e32 v[4:5], v[2:3]", "v_rsq_f64_e32 v[6:7], v[4:5]"]) == []           # (another transcendental: no forwarding hazard)


def test_every_kernel_the_library_ships_keeps_the_wait_states():
    """csrc/asm/*.fixed.s is what compile_unit.sh assembled into liblcp_hip.so; every unit of the Makefile, compiler-generated code and
    the hand-written statements alike, must be free of findings (the compiler pads its own instructions: a finding there would mean the
    check counts slots differently from the hardware rules it stands for)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the device assembly cannot be produced here")
    csrc = os.path.join(ROOT, "lcp_physics_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    units = [w[:-4] for w in mk.split("SRCS =")[1].split("\n")[0].split() if w.endswith(".hip")]
    missing = [u for u in units if not os.path.exists(os.path.join(csrc, "asm", u + ".fixed.s"))
               or os.path.getmtime(os.path.join(csrc, "asm", u + ".fixed.s")) < os.path.getmtime(os.path.join(csrc, u + ".hip"))]
    if missing:
        subprocess.run(["make", "-C", csrc, "-j8"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    nk = 0
    for u in units:
        lines = open(os.path.join(csrc, "asm", u + ".fixed.s")).read().split("\n")
        for name, lo, hi in isa_lint.kernels_of(lines):
            nk += 1
            out = []
            isa_lint.dpp_hazard(lines, name, lo, hi, quiet=out)
            assert out == [], (u, name, out[:3])
    assert nk >= 140, nk
