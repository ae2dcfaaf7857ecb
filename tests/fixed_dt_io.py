"""Shared loader of tests/golden/fixed_dt.npz (the reference `World` under `step(fixed_dt=True)`, tools/gen_fixed_dt_golden.py)."""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fixed_dt.npz")


@functools.lru_cache(maxsize=None)
def load_fixed_dt():
    """(worlds, rollout): `worlds[name]` = the record of one scene of part (a) (its fields as arrays), `rollout` = the `g_*`
    entries of part (b) without the prefix.  Read-only: loaded once and shared."""
    d = np.load(GOLD)
    names, keys, shapes = d["w_names"].tolist(), d["w_keys"].tolist(), d["w_shapes"]
    worlds = {n: {} for n in names}
    for j, k in enumerate(keys):
        flat, off = d["w_" + k], 0
        for i, n in enumerate(names):
            shp = tuple(int(x) for x in shapes[i, j, 1:1 + int(shapes[i, j, 0])])
            size = int(np.prod(shp)) if shp else 1
            a = flat[off:off + size].reshape(shp)
            worlds[n][k] = a
            off += size
        assert off == flat.size, k
    rollout = {k[2:]: d[k] for k in d.files if k.startswith("g_")}
    return worlds, rollout


def first_substep_of(rec):
    """Index into the flat sub-step arrays of the first sub-step of every step (and the total as the last entry)."""
    return np.concatenate([[0], np.cumsum(rec["nsub"])])
