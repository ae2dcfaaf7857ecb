"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the body
construction, lcp_body_properties_f64 and lcp_body_properties_backward_f64: guard bands around every buffer, const inputs bitwise
unchanged, each optional output NULL in turn, vertex slots >= nverts never read, outputs written and not accumulated."""
import os

import numpy as np
import pytest
import torch

from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INS = ("kind", "radius", "verts_raw", "nverts", "mass")
OUTS = ("centroid", "verts_local", "inertia", "Mdiag", "f_gravity", "bstatus")          # ("status" is the solvers' word in _check)
COTS = ("g_centroid", "g_verts_local", "g_inertia", "g_Mdiag", "g_f")
GRADS = ("g_verts_raw", "g_radius", "g_mass")


def _case(B, nb, cap, poison=None, twice=False):
    """The fixture's bodies of at most `cap` vertices, circles and hulls mixed, as B scenes of nb bodies; `poison`: the value of the
    vertex and cotangent slots >= nverts."""
    d = np.load(os.path.join(GOLDEN, "bodies.npz"))
    idx = np.nonzero(d["m_nverts"] <= cap)[0]
    idx = idx[np.random.default_rng(11).permutation(len(idx))]
    full = np.resize(idx, B * nb)
    t = lambda a, dt_: torch.tensor(a[full].reshape((B, nb) + a.shape[1:]), dtype=dt_)
    nv = t(d["m_nverts"], I32)
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    verts, gv = t(d["m_verts_raw"][:, :cap], F64), t(d["m_g_verts"][:, :cap], F64)
    if poison is not None:
        verts, gv = verts.masked_fill(pad, poison), gv.masked_fill(pad, poison)
    bufs = [("kind", I32, (B, nb), "in", t((d["m_kind"] != 0).astype(np.int32), I32)), ("radius", F64, (B, nb), "in", t(d["m_radius"], F64)),
            ("verts_raw", F64, (B, nb, cap, 2), "in", verts), ("nverts", I32, (B, nb), "in", nv), ("mass", F64, (B, nb), "in", t(d["m_mass"], F64)),
            ("centroid", F64, (B, nb, 2), "out", None), ("verts_local", F64, (B, nb, cap, 2), "out", None), ("inertia", F64, (B, nb), "out", None),
            ("Mdiag", F32, (B, nb, 3), "out", None), ("f_gravity", F32, (B, nb, 3), "out", None), ("bstatus", I32, (B, nb), "out", None),
            ("g_centroid", F64, (B, nb, 2), "in", t(d["m_g_centroid"], F64)), ("g_verts_local", F64, (B, nb, cap, 2), "in", gv),
            ("g_inertia", F64, (B, nb), "in", t(d["m_g_inertia"], F64)), ("g_Mdiag", F32, (B, nb, 3), "in", t(d["m_g_Mdiag"], F32)),
            ("g_f", F32, (B, nb, 3), "in", t(d["m_g_f"], F32)),
            ("g_verts_raw", F64, (B, nb, cap, 2), "out", None), ("g_radius", F64, (B, nb), "out", None), ("g_mass", F64, (B, nb), "out", None)]
    g = float(d["m_g"])
    steps = [Call("lcp_body_properties_f64", [B, nb, cap] + [R(n) for n in INS] + [g] + [R(n) for n in OUTS], OUTS),
             Call("lcp_body_properties_backward_f64", [B, nb, cap] + [R(n) for n in INS] + [g] + [R(n) for n in COTS + GRADS], GRADS)]

    def post(outs):
        assert int(outs["bstatus"].abs().max()) == 0
        for n in ("verts_local", "g_verts_raw"):
            assert _absmax(outs[n][pad]) == 0.0, (n, "slots >= nverts are not zero")
        circ = t((d["m_kind"] == 0), torch.bool)
        assert _absmax(outs["g_radius"][~circ]) == 0.0 and _absmax(outs["centroid"][circ]) == 0.0

    # each optional output of either call NULL in turn (the cotangents: test_null_cotangents_are_zeros)
    nulls = [{n} for n in OUTS + GRADS]
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post)


@pytest.mark.parametrize("B,nb,cap", [(3, 1, 8), (3, 5, 8), (3, 33, 16), (3, 5, 64), (1, 3, 12)])
def test_guards_optional_outputs_and_buffer_neighbourhood(B, nb, cap):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn (B x nb x lanes-per-body is no multiple of the 256-thread block at any
    of these sizes: tail bodies; cap = 12: a capacity that is no power of two)."""
    _check(_case(B, nb, cap))


@pytest.mark.parametrize("cap", [8, 16, 64])
def test_slots_beyond_nverts_are_never_read(cap):
    """Input vertex and cotangent slots >= nverts poisoned with NaN: every output finite and bit for bit what zeros there give."""
    clean = _check(_case(3, 5, cap))
    dirty = _check(_case(3, 5, cap, poison=float("nan")))
    for n in clean:
        assert _same(clean[n], dirty[n]), n


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case(3, 5, 16))
    twice, _, _ = _run(_case(3, 5, 16, twice=True))
    for n in once:
        assert _same(once[n], twice[n]), n
    assert float(once["g_mass"].abs().min()) > 0.0 and float(once["inertia"].min()) > 0.0


def test_null_cotangents_are_zeros():
    """Each cotangent NULL gives the bits of that cotangent filled with zeros."""
    base = _case(3, 5, 16)
    for c in COTS:
        null, _, _ = _run(base, null=frozenset({c}))
        zero = _case(3, 5, 16)
        zero.bufs = [(n, dt_, sh, role, torch.zeros(sh, dtype=dt_) if n == c else data) for n, dt_, sh, role, data in zero.bufs]
        want, _, _ = _run(zero)
        for n in GRADS:
            assert _same(null[n], want[n]), (c, n)


def test_refusals_write_nothing():
    """A NULL required pointer or a capacity outside 8 .. 64: LCP_E_BADARG and no output touched; B = 0: success and no output touched."""
    case = _case(3, 5, 16)
    ins = [R(n) for n in INS]
    g = 100.0
    bad_in = ins[:2] + [R("verts_missing")] + ins[3:]
    case.steps = [Call("lcp_body_properties_f64", [3, 5, 16] + bad_in + [g] + [R(n) for n in OUTS], OUTS, rc=-1),
                  Call("lcp_body_properties_f64", [3, 5, 7] + ins + [g] + [R(n) for n in OUTS], OUTS, rc=-1),
                  Call("lcp_body_properties_f64", [3, 5, 65] + ins + [g] + [R(n) for n in OUTS], OUTS, rc=-1),
                  Call("lcp_body_properties_backward_f64", [3, 5, 16] + bad_in + [g] + [R(n) for n in COTS + GRADS], GRADS, rc=-1),
                  Call("lcp_body_properties_backward_f64", [3, 5, 66] + ins + [g] + [R(n) for n in COTS + GRADS], GRADS, rc=-1)]
    _run(case)
    empty = _case(3, 5, 16)
    empty.steps = [Call("lcp_body_properties_f64", [0, 5, 16] + ins + [g] + [R(n) for n in OUTS], OUTS),
                   Call("lcp_body_properties_backward_f64", [3, 0, 16] + ins + [g] + [R(n) for n in COTS + GRADS], GRADS)]
    outs, _, _ = _run(empty)
    for n in OUTS + GRADS:
        assert bool((outs[n].contiguous().view(-1).view(torch.uint8) == 0xFF).all()), n
