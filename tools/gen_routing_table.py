"""Record the host routing table that tests/test_routing_table.py replays: lcp_workspace_bytes, lcp_step_has_backward and
lcp_post_stabilization_has_backward over sizes around every kernel family's boundary and over the `compute` words that steer
the routing (arithmetic, I/O type, each LCP_PATH_* bit, the hints, the thread's lcp_debug_set_path default).

    python tools/gen_routing_table.py [out.npz]        (LCP_HIP_LIB selects the library, see lcp_physics_amd/_lib.py)

Host-only: the three queries never touch a GPU.  The file holds the sweep's axes and one result per point of their product:
`ws[nz, contacts, e, B, ws_word]` (lcp_workspace_bytes) and `bwd[query, nb, contacts, e, word]` (0: lcp_step_has_backward,
1: lcp_post_stabilization_has_backward), a word being (`compute` bits, lcp_debug_set_path default)."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lcp_physics_amd import _lib  # noqa: E402

CONTACTS = (4, 16, 17, 32, 33, 64, 65, 256, 257)
EQ = (0, 3, 4, 5, 8, 24, 25)
TOTALS = (20, 24, 40, 56, 64, 128, 129)            # nz + e
BATCHES = (1, 63, 64, 65)                          # the per-scene class words pad B * 4 bytes to 256
PATH_BITS = (_lib.PATH_GENERIC, _lib.PATH_CONTACT_SPACE, _lib.PATH_PRIMAL, _lib.PATH_PRIMAL_WG, _lib.PATH_QUAD, _lib.PATH_SOLO)
HINTS = (_lib.HINT_PINNED, _lib.HINT_ALL_CONTACT, _lib.IO_F64, _lib.BWD_ADJOINT, _lib.HINT_PINNED | _lib.PATH_PRIMAL_WG,
         _lib.HINT_PINNED | _lib.PATH_CONTACT_SPACE)
THREAD_PATHS = (1, 2, 3, 4, 5)                     # lcp_debug_set_path defaults, for words without path bits


def axes():
    nz = sorted({15, 16, 17, 30, 32, 33} | {t - e for t in TOTALS for e in EQ if t - e > 0})
    nb = sorted({5, 6, 10, 11} | {(t - e) // 3 + d for t in TOTALS for e in EQ for d in (0, 1) if (t - e) // 3 + d > 0})
    ws_words = [(a, 0) for a in (_lib.COMPUTE_F32, _lib.COMPUTE_F64, _lib.COMPUTE_F64 | _lib.IO_F64, _lib.COMPUTE_F32 | _lib.IO_F64)]
    words = []
    for a in (_lib.COMPUTE_F32, _lib.COMPUTE_F64):
        words += [(a, 0)] + [(a | b, 0) for b in PATH_BITS + HINTS]
        words += [(a, tp) for tp in THREAD_PATHS] + [(a | _lib.HINT_PINNED, tp) for tp in THREAD_PATHS]
    return {"nz": np.array(nz), "nb": np.array(nb), "contacts": np.array(CONTACTS), "e": np.array(EQ), "B": np.array(BATCHES),
            "ws_words": np.array(ws_words), "words": np.array(words)}


def with_thread_path(lib, tp, fn):
    lib.lcp_debug_set_path(int(tp))
    try:
        return fn()
    finally:
        lib.lcp_debug_set_path(0)


def record(lib, ax):
    """The two result arrays for the axes `ax` (also what the test computes from the library under test)."""
    ws = np.zeros((len(ax["nz"]), len(ax["contacts"]), len(ax["e"]), len(ax["B"]), len(ax["ws_words"])), dtype=np.int64)
    bwd = np.zeros((2, len(ax["nb"]), len(ax["contacts"]), len(ax["e"]), len(ax["words"])), dtype=np.int8)
    fns = (lib.lcp_step_has_backward, lib.lcp_post_stabilization_has_backward)
    for (i, nz), (j, c), (k, e), (l, B), (w, (word, tp)) in _product(ax, ("nz", "contacts", "e", "B", "ws_words")):
        ws[i, j, k, l, w] = with_thread_path(lib, tp, lambda: lib.lcp_workspace_bytes(int(B), int(nz), 4 * int(c), int(e), int(word)))
    for q in (0, 1):
        for (i, nb), (j, c), (k, e), (w, (word, tp)) in _product(ax, ("nb", "contacts", "e", "words")):
            bwd[q, i, j, k, w] = with_thread_path(lib, tp, lambda: fns[q](int(nb), int(c), int(e), int(word)))
    return ws, bwd


def _product(ax, names):
    return itertools.product(*[list(enumerate(ax[n])) for n in names])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "routing_table.npz")
    ax = axes()
    ws, bwd = record(_lib.load(), ax)
    np.savez_compressed(out, ws=ws, bwd=bwd, **ax)
    print("%d + %d entries -> %s (%d bytes)" % (ws.size, bwd.size, out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
