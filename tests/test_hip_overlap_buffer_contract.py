"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the overlap
queries, lcp_pair_overlap_f64 and lcp_pair_overlap_backward_f64: guard bands around every buffer, const inputs bitwise unchanged,
each optional output NULL in turn, vertex slots >= nverts never read, outputs written and not accumulated, the same bits with the
arena carved in reverse."""
import pytest
import torch

from tests import overlap_host as OH
from tests.test_hip_buffer_contract import F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = ("kind", "radius", "verts_local", "nverts", "p", "pair_first", "pair_second")
OUTS = ("area",)
GRADS = ("g_p", "g_radius", "g_verts_local")


def _case(name, poison=None, twice=False):
    """Case `name` of overlap_host.py; `poison`: the value of the vertex slots >= nverts."""
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in OH.case(name).items()}
    B, nb, cap = c["verts_local"].shape[:3]
    npair = c["pair_first"].shape[1]
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    if poison is not None:
        c["verts_local"] = c["verts_local"].masked_fill(pad, poison)
    ref = OH.reference(name)
    bufs = [("kind", I32, (B, nb), "in", c["kind"]), ("radius", F64, (B, nb), "in", c["radius"]),
            ("verts_local", F64, (B, nb, cap, 2), "in", c["verts_local"]), ("nverts", I32, (B, nb), "in", c["nverts"]),
            ("p", F64, (B, nb, 3), "in", c["p"]), ("pair_first", I32, (B, npair), "in", c["pair_first"]),
            ("pair_second", I32, (B, npair), "in", c["pair_second"]), ("g_area", F64, (B, npair), "in", ref["g_area"]),
            ("area", F64, (B, npair), "out", None),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_radius", F64, (B, nb), "out", None),
            ("g_verts_local", F64, (B, nb, cap, 2), "out", None)]
    sizes = [B, nb, cap, int(nv.sum(1).max()), npair]
    steps = [Call("lcp_pair_overlap_f64", sizes + [R(n) for n in INS] + [R(n) for n in OUTS], OUTS),
             Call("lcp_pair_overlap_backward_f64", sizes + [R(n) for n in INS] + [R("g_area")] + [R(n) for n in GRADS], GRADS)]

    def post(outs):
        assert _absmax(outs["area"] - ref["area"]) <= 1e-9
        assert _absmax(outs["g_verts_local"][pad]) == 0.0, "slots >= nverts are not zero"
        assert _absmax(outs["g_radius"][hull]) == 0.0 and _absmax(outs["g_p"]) > 0.0

    nulls = [{n} for n in GRADS] + [{"g_p", "g_radius"}]              # each optional output NULL in turn (area is required)
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post), sizes


@pytest.mark.parametrize("name", ["tiny", "small", "wide"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn ("tiny": one pair of one scene; "small": every kind of pair; "wide": 276
    pairs, more than one chunk of 256 and no multiple of a wavefront)."""
    _check(_case(name)[0])


@pytest.mark.parametrize("name", ["small", "wide"])
def test_slots_beyond_nverts_are_never_read(name):
    """Vertex slots >= nverts (all of a circle's) poisoned with NaN: every output finite and bit for bit what zeros there give."""
    clean, _, _ = _run(_case(name)[0])
    dirty, _, _ = _run(_case(name, poison=float("nan"))[0])
    for n in clean:
        assert _same(clean[n], dirty[n]), n
        assert bool(torch.isfinite(dirty[n].double()).all()), n


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("small")[0])
    twice, _, _ = _run(_case("small", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """A NULL required pointer, sizes outside the limits: LCP_E_BADARG and no output touched."""
    case, sizes = _case("small")
    ins = [R(n) for n in INS]
    outs, grads = [R(n) for n in OUTS], [R("g_area")] + [R(n) for n in GRADS]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    case.steps = [Call("lcp_pair_overlap_backward_f64", sizes + ins + [R("g_missing")] + grads[1:], GRADS, rc=-1),
                  Call("lcp_pair_overlap_f64", sizes + ins + [R("missing")], OUTS, rc=-1)]
    for k in range(len(INS)):
        bad_in = ins[:k] + [R("missing")] + ins[k + 1:]
        case.steps += [Call("lcp_pair_overlap_f64", sizes + bad_in + outs, OUTS, rc=-1),
                       Call("lcp_pair_overlap_backward_f64", sizes + bad_in + grads, GRADS, rc=-1)]
    for k, v in ((0, -1), (1, 0), (1, 65), (2, 7), (2, 65), (3, -1), (3, 1025), (4, 0), (4, 1025)):
        case.steps += [Call("lcp_pair_overlap_f64", with_size(k, v) + ins + outs, OUTS, rc=-1),
                       Call("lcp_pair_overlap_backward_f64", with_size(k, v) + ins + grads, GRADS, rc=-1)]
    _run(case)
