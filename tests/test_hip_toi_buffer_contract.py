"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the
time-of-impact query, lcp_time_of_impact_f64 and lcp_time_of_impact_backward_f64: guard bands around every buffer, const inputs
bitwise unchanged, each optional output NULL in turn, vertex slots >= nverts never read, outputs written and not accumulated, the same
bits with the arena carved in reverse."""
import pytest
import torch

from tests import toi_host as TH
from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = ("kind", "radius", "verts_local", "nverts", "p", "v", "pair_first", "pair_second")
OUTS = ("toi", "status", "normal", "first_toi", "first_pair")
GRADS = ("g_p", "g_v", "g_radius", "g_verts_local", "g_margin")


def _case(name, poison=None, twice=False):
    """Case `name` of toi_host.py through both entries, the backward on the forward's own toi and status; `poison`: the value of the
    vertex slots >= nverts."""
    c = dict(TH.case(name))
    B, nb, cap = c["verts_local"].shape[:3]
    npair = c["pair_first"].shape[1]
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    if poison is not None:
        c["verts_local"] = c["verts_local"].masked_fill(pad, poison)
    ref = TH.reference(name)
    g = torch.randn(B, npair, generator=torch.Generator().manual_seed(3), dtype=F64)
    bufs = [("kind", I32, (B, nb), "in", c["kind"]), ("radius", F64, (B, nb), "in", c["radius"]),
            ("verts_local", F64, (B, nb, cap, 2), "in", c["verts_local"]), ("nverts", I32, (B, nb), "in", c["nverts"]),
            ("p", F64, (B, nb, 3), "in", c["p"]), ("v", F32, (B, nb, 3), "in", c["v"]),
            ("pair_first", I32, (B, npair), "in", c["pair_first"]), ("pair_second", I32, (B, npair), "in", c["pair_second"]),
            ("margin", F64, (B, npair), "in", c["margin"]), ("horizon", F64, (B,), "in", c["horizon"]), ("g_toi", F64, (B, npair), "in", g),
            ("toi", F64, (B, npair), "out", None), ("status", I32, (B, npair), "out", None), ("normal", F64, (B, npair, 2), "out", None),
            ("first_toi", F64, (B,), "out", None), ("first_pair", I32, (B,), "out", None),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_v", F64, (B, nb, 3), "out", None), ("g_radius", F64, (B, nb), "out", None),
            ("g_verts_local", F64, (B, nb, cap, 2), "out", None), ("g_margin", F64, (B, npair), "out", None)]
    sizes = [B, nb, cap, c.get("svm", int(nv.sum(1).max())), npair]
    ins = [R(n) for n in INS]
    steps = [Call("lcp_time_of_impact_f64", sizes + ins + [R("margin"), R("horizon"), c["tol"], c["max_iter"]] + [R(n) for n in OUTS], OUTS),
             Call("lcp_time_of_impact_backward_f64", sizes + ins + [R("toi"), R("status"), R("g_toi")] + [R(n) for n in GRADS], GRADS)]

    def post(outs):
        keep = ~ref["excluded"]
        assert torch.equal(outs["status"][keep], ref["status"][keep])
        assert _absmax(outs["g_verts_local"][pad]) == 0.0, "slots >= nverts are not zero"
        assert _absmax(outs["g_radius"][hull]) == 0.0
        if name != "notqueried":
            assert _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_v"]) > 0.0 and bool((outs["first_pair"] >= 0).all())

    # each optional output of either call NULL in turn (the backward runs on the forward's toi and status: those two stay)
    nulls = [{n} for n in ("normal", "first_toi", "first_pair") + GRADS]
    unwritten = {"first_pair": [0, 1]} if name == "notqueried" else None          # (-1, no pair: what the arena's fill reads as, too)
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post, unwritten=unwritten), sizes


@pytest.mark.parametrize("name", ["mixed", "edges257", "edges1024", "notqueried"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn ("mixed": 10 pairs; "edges257": one pair more than a pass of 256, with the
    invalid pairs; "edges1024": the most pairs, the largest LDS the backward can ask for at this capacity; "notqueried": a scene over
    scene_verts_max and one with a horizon of 0)."""
    _check(_case(name)[0])


def test_toi_and_status_alone():
    """The forward with only toi, only status: the bits of the full call."""
    case, _ = _case("edges65")
    full, _, _ = _run(case)
    case.steps = case.steps[:1]
    for keep in ("toi", "status"):
        part, _, _ = _run(case, null=frozenset(set(OUTS + GRADS) - {keep}))
        assert _same(part[keep], full[keep]), keep


@pytest.mark.parametrize("name", ["mixed", "edges65"])
def test_slots_beyond_nverts_are_never_read(name):
    """Vertex slots >= nverts (all of a circle's) poisoned with NaN: every output finite and bit for bit what zeros there give."""
    clean, _, _ = _run(_case(name)[0])
    dirty, _, _ = _run(_case(name, poison=float("nan"))[0])
    for n in clean:
        assert _same(clean[n], dirty[n]), n
        assert bool(torch.isfinite(dirty[n].double()).all()), n


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("mixed")[0])
    twice, _, _ = _run(_case("mixed", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """A NULL required pointer, sizes and scalars outside the limits: LCP_E_BADARG and no output touched."""
    case, sizes = _case("mixed")
    c = TH.case("mixed")
    ins = [R(n) for n in INS]
    tail = [R("margin"), R("horizon"), c["tol"], c["max_iter"]]
    outs, grads = [R(n) for n in OUTS], [R(n) for n in GRADS]
    state = [R("toi_in"), R("status_in"), R("g_toi")]
    case.bufs += [("toi_in", F64, case.bufs[11][2], "in", torch.zeros(case.bufs[11][2], dtype=F64)),
                  ("status_in", I32, case.bufs[12][2], "in", torch.ones(case.bufs[12][2], dtype=I32))]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    fwd = lambda s, i, t: Call("lcp_time_of_impact_f64", s + i + t + outs, OUTS, rc=-1)
    bwd = lambda s, i, st: Call("lcp_time_of_impact_backward_f64", s + i + st + grads, GRADS, rc=-1)
    case.steps = [bwd(sizes, ins, [R("missing")] + state[1:]), bwd(sizes, ins, state[:1] + [R("missing")] + state[2:]),
                  bwd(sizes, ins, state[:2] + [R("missing")]), fwd(sizes, ins, [R("missing")] + tail[1:]),
                  fwd(sizes, ins, tail[:1] + [R("missing")] + tail[2:]), fwd(sizes, ins, tail[:2] + [0.0, 64]),
                  fwd(sizes, ins, tail[:2] + [1e-6, 0]), fwd(sizes, ins, tail[:2] + [1e-6, 1025])]
    for k in range(len(INS)):
        bad_in = ins[:k] + [R("missing")] + ins[k + 1:]
        case.steps += [fwd(sizes, bad_in, tail), bwd(sizes, bad_in, state)]
    for k, v in ((0, -1), (1, 0), (1, 65), (2, 7), (2, 65), (3, -1), (3, 1025), (4, 0), (4, 1025)):
        case.steps += [fwd(with_size(k, v), ins, tail), bwd(with_size(k, v), ins, state)]
    _run(case)
