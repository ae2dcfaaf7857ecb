"""Per-phase cycle breakdown of the four-scenes-per-wave forward kernel of the contact-list entry points (the kernel bench.py
times).  Needs the -DLCP_Q_PROFILE build:
    make -C lcp_physics_amd/csrc quadprof
    LCP_HIP_LIB=tools/liblcp_quadprof.so python tools/gpu_phase_profile_quad.py [B] [nbox]
(the profiling build writes the cycle record of a wave over the tail of its first scene's `s` output; the dense backward
lcp_bwd_quad writes its own over the tail of the scene's `dh` row)."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lcp_physics_amd import scenes
from lcp_physics_amd.physics import fused_step
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
nbox = int(sys.argv[2]) if len(sys.argv) > 2 else 4
sc = scenes.make_stack_scenes(B=B, nbox=nbox, pts_per_interface=4, seed=1236, dtype=torch.float32).to(device="cuda")
out = None
for rep in range(3):
    out = fused_step(sc, out=out, ws=None if out is None else out["ws"])
    torch.cuda.synchronize()
t = out["s"][::4, -21:].double().cpu()           # one record per wave (lane 0 = first scene of the wave)
names = ["residuals + d", "factor: formation", "factor: LU", "solve_kkt: products before", "solve_kkt: triangular sweeps",
         "solve_kkt: products after", "bookkeeping / best iterate", "step lengths, sigma, update"]
tot = t[:, :8].sum(1)
print("B=%d nbox=%d  mean cycles per wave (clock64 ticks): total of the phases %.0f   (iters %.1f)   prologue %.0f   whole kernel (first to last instruction of the wave) %.0f" % (
    B, nbox, tot.mean(), t[:, 8].mean(), t[:, 9].mean(), t[:, 10].mean()))
print("  prologue: kernel start -> every input loaded and assembled %.0f, -> LDS barrier + Jacobian columns to registers %.0f, -> loop %.0f" % (
    t[:, 11].mean(), t[:, 12].mean(), (t[:, 9] - t[:, 11] - t[:, 12]).mean()))
for k, n in enumerate(names):
    print("  %-32s mean %10.0f  (%.1f%%)" % (n, t[:, k].mean(), 100 * t[:, k].mean() / tot.mean()))
# the stretch before the loop in six parts, and first trips through the code against hot ones
ack = t[:, 11] - t[:, 13] - t[:, 14] - t[:, 15] - t[:, 19]
loop_in = t[:, 9] - t[:, 11] - t[:, 12]
print("  prologue in parts: start -> loads issued %.0f, -> arrived %.0f, -> contact records built %.0f, -> rows in registers %.0f, "
      "(-> the stamp's own wait for the meta stores' acknowledgement %.0f: not spent by the kernel proper), -> columns and masks %.0f, "
      "-> loop entry %.0f" % (t[:, 13].mean(), t[:, 14].mean(), t[:, 15].mean(), t[:, 19].mean(), ack.mean(), t[:, 12].mean(), loop_in.mean()))
hot = t[:, 18] / (t[:, 8] - 1).clamp(min=1)
print("  first trips: initialisation pass %.0f, iteration 0 %.0f; hot trips: iterations 1.. %.0f each (%.1f of them)" % (
    t[:, 16].mean(), t[:, 17].mean(), hot.mean(), (t[:, 8] - 1).mean()))
# the dense backward behind it
from lcp_physics_amd.lcp import lcp_backward
from lcp_physics_amd.physics import assemble_contacts
from lcp_physics_amd.physics.batched_world import solution_of_step
lcp = assemble_contacts(sc)
sol = solution_of_step(sc, out, lcp[2], lcp[4])
cot = torch.randn(B, lcp[0].shape[1], generator=torch.Generator().manual_seed(4321)).to("cuda")
grads = None
for rep in range(3):
    grads = lcp_backward(sol, cot, out=grads)
    torch.cuda.synchronize()
b = grads[3][::4, -6:].double().cpu()            # [dQ, dp, dG, dh, dA, db, dF]: one record per wave in dh
segs = ["start -> loads issued", "-> arrived", "-> staged + barrier", "-> solve done", "-> last store issued", "-> end"]
prev = torch.zeros(b.shape[0], dtype=torch.float64)
print("lcp_bwd_quad: mean cycles per wave, whole kernel %.0f" % b[:, 5].mean())
for k, n in enumerate(segs):
    print("  %-24s %8.0f   (at %.0f)" % (n, (b[:, k] - prev).mean(), b[:, k].mean()))
    prev = b[:, k]
