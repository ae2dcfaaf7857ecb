"""Generate tests/golden/engine_scenes.npz by running the UNMODIFIED reference op (`LCPFunction`, through
oracle/ref_shim.py) one scene at a time (batch 1) on seeded synthetic stack scenes.  TEST INFRASTRUCTURE ONLY;
needs the reference tree.

    PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_engine_scenes.py

Stored: the dense LCP the reference was given (in_Q .. in_F, float64, batched over the scenes) and its solution
(x, lams, slacks).  tests/test_oracle_golden.py::test_oracle_matches_live_reference_on_random_engine_scenes
pins the vectorised oracle against these.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pdipm_oracle as O  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
# the scenes of the test: make_stack_scenes(B=6, nbox=2, pts_per_interface=2, seed=11, float64)
B, NBOX, PTS, SEED = 6, 2, 2, 11


def main():
    mods = ref_shim.load_reference()
    from lcp_physics_amd import scenes
    sc = scenes.make_stack_scenes(B=B, nbox=NBOX, pts_per_interface=PTS, seed=SEED, dtype=torch.float64)
    lcp = O.assemble_lcp(*sc.assembly_args())
    xs, lams, slacks = [], [], []
    for i in range(B):
        fn = mods["engines"].LCPFunction(max_iter=10, verbose=-1)
        x = fn(*[t[i:i + 1] for t in lcp])
        xs.append(x.detach())
        lams.append(fn.lams.detach())
        slacks.append(fn.slacks.detach())
    out = {"in_" + nm: t.numpy() for nm, t in zip("QpGhAbF", lcp)}
    out.update(x=torch.cat(xs).numpy(), lams=torch.cat(lams).numpy(), slacks=torch.cat(slacks).numpy(),
               scenes=np.array([B, NBOX, PTS, SEED], dtype=np.int64))
    np.savez_compressed(os.path.join(OUT, "engine_scenes.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
