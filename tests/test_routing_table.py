"""Host routing table: lcp_workspace_bytes, lcp_step_has_backward and lcp_post_stabilization_has_backward answer, over sizes around
every kernel family's boundary and over the `compute` words that steer the routing, what the table recorded by
tools/gen_routing_table.py holds (tests/golden/routing_table.npz: the sweep's axes and one result per point).  Host-only: no GPU."""
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routing_table.npz")


def _points(t, names):
    return itertools.product(*[list(enumerate(t[n])) for n in names])


def test_host_routing_matches_the_recorded_table():
    from lcp_physics_amd import _lib
    lib = _lib.load()
    with np.load(GOLDEN) as f:
        t = {k: f[k] for k in f.files}

    def at(tp, fn, *args):
        lib.lcp_debug_set_path(int(tp))
        try:
            return int(fn(*(int(a) for a in args)))
        finally:
            lib.lcp_debug_set_path(0)

    n = 0
    for (i, nz), (j, c), (k, e), (l, B), (w, (word, tp)) in _points(t, ("nz", "contacts", "e", "B", "ws_words")):
        got, want = at(tp, lib.lcp_workspace_bytes, B, nz, 4 * c, e, word), int(t["ws"][i, j, k, l, w])
        assert got == want, "lcp_workspace_bytes(B=%d, nz=%d, m=%d, e=%d, 0x%x) = %d, recorded %d" % (B, nz, 4 * c, e, word, got, want)
        n += 1
    for q, fn in enumerate((lib.lcp_step_has_backward, lib.lcp_post_stabilization_has_backward)):
        for (i, nb), (j, c), (k, e), (w, (word, tp)) in _points(t, ("nb", "contacts", "e", "words")):
            got, want = at(tp, fn, nb, c, e, word), int(t["bwd"][q, i, j, k, w])
            assert got == want, "%s(nb=%d, maxc=%d, e=%d, 0x%x) with lcp_debug_set_path(%d) = %d, recorded %d" % (
                fn.__name__, nb, c, e, word, tp, got, want)
            n += 1
    assert n == t["ws"].size + t["bwd"].size
