"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the point
probes, lcp_point_distance_f64 and lcp_point_distance_backward_f64: guard bands around every buffer, const inputs bitwise unchanged,
each optional output NULL in turn, vertex slots >= nverts never read, outputs written and not accumulated, the same bits with the arena
carved in reverse."""
import pytest
import torch

from tests import points_host as PH
from tests.test_hip_buffer_contract import F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = ("kind", "radius", "verts_local", "nverts", "p", "pt_body", "pt_xy", "pt_target", "pt_max_dist")
OUTS = ("dist", "body", "normal")
GRADS = ("g_p", "g_radius", "g_verts_local", "g_pt_xy")
CASES = ("small", "wide")
FAR = 1e4                        # stands for max_dist = inf: the arena's check reads a written element as a finite one


def _case(name, poison=None, twice=False):
    """Case `name` of points_host.py with every infinite max_dist replaced by FAR (no point of the cases is that far from a body, so
    the selections are the mirror's); `poison`: the value of the vertex slots >= nverts.  -1 is a value of `body` (a void point), which
    the arena's fill reads as "not written": `body` is pre-filled with -7 instead and checked by `post`."""
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in PH.case(name).items()}
    c["pt_max_dist"] = c["pt_max_dist"].clamp(max=FAR)
    B, nb, cap = c["verts_local"].shape[:3]
    n = c["pt_body"].shape[1]
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    if poison is not None:
        c["verts_local"] = c["verts_local"].masked_fill(pad, poison)
    ref = PH.reference(name)
    g = ref["g_dist"]
    bufs = [("kind", I32, (B, nb), "in", c["kind"]), ("radius", F64, (B, nb), "in", c["radius"]),
            ("verts_local", F64, (B, nb, cap, 2), "in", c["verts_local"]), ("nverts", I32, (B, nb), "in", c["nverts"]),
            ("p", F64, (B, nb, 3), "in", c["p"]), ("pt_body", I32, (B, n), "in", c["pt_body"]),
            ("pt_xy", F64, (B, n, 2), "in", c["pt_xy"]), ("pt_target", I32, (B, n), "in", c["pt_target"]),
            ("pt_max_dist", F64, (B, n), "in", c["pt_max_dist"]), ("g_dist", F64, (B, n), "in", g),
            ("dist", F64, (B, n), "out", None), ("body", I32, (B, n), "inout", torch.full((B, n), -7, dtype=I32)),
            ("normal", F64, (B, n, 2), "out", None),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_radius", F64, (B, nb), "out", None),
            ("g_verts_local", F64, (B, nb, cap, 2), "out", None), ("g_pt_xy", F64, (B, n, 2), "out", None)]
    sizes = [B, nb, cap, int(nv.sum(1).max()), n]
    steps = [Call("lcp_point_distance_f64", sizes + [R(k) for k in INS] + [R(k) for k in OUTS], OUTS),
             Call("lcp_point_distance_backward_f64", sizes + [R(k) for k in INS] + [R("g_dist")] + [R(k) for k in GRADS], GRADS)]

    def post(outs):
        if "body" in outs:                                            # (-1 is a value of `body`: written means no -7 is left)
            assert int(outs["body"].min()) >= -1 and int(outs["body"].max()) < nb
            keep = ~ref["excluded"]
            assert torch.equal(outs["body"][keep], ref["body"][keep])
            void = outs["body"] < 0
            assert torch.equal(outs["dist"][void], c["pt_max_dist"][void]) and _absmax(outs["normal"][void]) == 0.0
        assert _absmax(outs["g_verts_local"][pad]) == 0.0, "slots >= nverts are not zero"
        assert _absmax(outs["g_radius"][hull]) == 0.0 and _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_pt_xy"]) > 0.0

    nulls = [{k} for k in OUTS + GRADS]                               # each optional output of either call NULL in turn
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post, unwritten={"body": range(B)}), sizes


@pytest.mark.parametrize("name", CASES)
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn ("small": 70 points, more than a wavefront and no multiple of one; "wide":
    the largest scene, the most points, the largest LDS either kernel can ask for)."""
    _check(_case(name)[0])


@pytest.mark.parametrize("name", CASES)
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
    case.bufs = [b if b[0] != "body" else ("body", I32, b[2], "out", None) for b in case.bufs]
    ins = [R(n) for n in INS]
    outs, grads = [R(n) for n in OUTS], [R("g_dist")] + [R(n) for n in GRADS]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    case.steps = [Call("lcp_point_distance_backward_f64", sizes + ins + [R("g_missing")] + grads[1:], GRADS, rc=-1)]
    for k in range(len(INS)):
        bad_in = ins[:k] + [R("missing")] + ins[k + 1:]
        case.steps += [Call("lcp_point_distance_f64", sizes + bad_in + outs, OUTS, rc=-1),
                       Call("lcp_point_distance_backward_f64", sizes + bad_in + grads, GRADS, rc=-1)]
    for k, v in ((0, -1), (1, 0), (1, 65), (2, 7), (2, 65), (3, -1), (3, 1025), (4, 0), (4, 1025)):
        case.steps += [Call("lcp_point_distance_f64", with_size(k, v) + ins + outs, OUTS, rc=-1),
                       Call("lcp_point_distance_backward_f64", with_size(k, v) + ins + grads, GRADS, rc=-1)]
    _run(case)
