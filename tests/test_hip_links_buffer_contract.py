"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the mechanism
links, lcp_link_jacobian_f64 and lcp_link_jacobian_backward_f64: guard bands around every buffer, const inputs bitwise unchanged, every
output fully written, each optional buffer NULL in turn, outputs written and not accumulated, the same bits with the arena carved in
reverse, refusals that write nothing - and kind-0 links and out-of-range body indices that write zero rows and nothing else."""
import pytest
import torch

from tests import links_host as LH
from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = LH.LINK_ARRAYS + ("p",)
GRADS = tuple("g_" + n for n in LH.LEAVES)
E0 = 3


def _case(name, twice=False):
    c, ref = LH.case(name), LH.reference(name)
    B, nb = c["p"].shape[:2]
    L, el = c["kind"].shape[1], LH.el_of(c["kind"])
    base = torch.zeros(B, E0, 3 * nb, dtype=F32)
    base[:, :, :3] = torch.eye(3)
    gJe = torch.cat([torch.randn(B, E0, 3 * nb, generator=torch.Generator().manual_seed(9)), c["g_Je"]], 1)
    shape = lambda n: (B, L, 2) if n in ("a1", "a2") else (B, L)
    bufs = [(n, I32 if n in ("kind", "first", "second") else F64, shape(n), "in", c[n]) for n in LH.LINK_ARRAYS]
    bufs += [("p", F64, (B, nb, 3), "in", c["p"]), ("Je_base", F32, (B, E0, 3 * nb), "in", base),
             ("g_Je", F32, (B, E0 + el, 3 * nb), "in", gJe), ("Je", F32, (B, E0 + el, 3 * nb), "out", None)]
    bufs += [("g_" + n, F64, (B, nb, 3) if n == "p" else shape(n), "out", None) for n in LH.LEAVES]
    sizes = [B, nb, L, E0, el]
    steps = [Call("lcp_link_jacobian_f64", sizes + [R(n) for n in INS] + [R("Je_base"), R("Je")], ("Je",)),
             Call("lcp_link_jacobian_backward_f64", sizes + [R(n) for n in INS] + [R("g_Je")] + [R(n) for n in GRADS], GRADS)]

    def post(outs):
        assert _same(outs["Je"][:, :E0], base)
        rows = outs["Je"][:, E0:]
        assert _absmax(rows.double() - ref["Je"]) <= 2.0 ** -23 * _absmax(ref["Je"])
        assert _absmax(rows[~ref["struct"]]) == 0.0 and _absmax(rows[~ref["live"]]) == 0.0    # kind 0, bad indices: zero rows, no more
        assert _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_p"] - ref["grads"]["p"]) <= 1e-9 * _absmax(ref["grads"]["p"])

    nulls = [{n} for n in GRADS]                                      # each optional gradient NULL in turn
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post), sizes


@pytest.mark.parametrize("name", ["mixed", "many_scenes", "many_links", "invalid"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional gradient NULL in turn ("mixed": several scenes in one wavefront; "many_scenes": a last
    workgroup with empty groups; "many_links": a group of 128 lanes; "invalid": kind 0, unknown kinds and body indices out of range
    between live links)."""
    _check(_case(name)[0])


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("mixed")[0])
    twice, _, _ = _run(_case("mixed", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """A NULL required pointer, sizes outside the limits, no output: refused and no output touched."""
    case, sizes = _case("mixed")
    ins = [R(n) for n in INS]
    fwd_tail, grads = [R("Je_base"), R("Je")], [R("g_Je")] + [R(n) for n in GRADS]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    case.steps = [Call("lcp_link_jacobian_backward_f64", sizes + ins + [R("g_missing")] + grads[1:], GRADS, rc=-1),
                  Call("lcp_link_jacobian_backward_f64", sizes + ins + [R("g_Je")] + [R("missing")] * 4, GRADS, rc=-1),
                  Call("lcp_link_jacobian_f64", sizes + ins + [R("Je_base"), R("missing")], ("Je",), rc=-1),
                  Call("lcp_link_jacobian_f64", sizes + ins + [R("missing"), R("Je")], ("Je",), rc=-1)]
    for k in range(len(INS)):
        bad_in = ins[:k] + [R("missing")] + ins[k + 1:]
        case.steps += [Call("lcp_link_jacobian_f64", sizes + bad_in + fwd_tail, ("Je",), rc=-1),
                       Call("lcp_link_jacobian_backward_f64", sizes + bad_in + grads, GRADS, rc=-1)]
    for k, v, rc in ((0, -1, -1), (1, 0, -1), (1, 65, -2), (2, 0, -1), (2, 257, -2), (3, -1, -1), (3, 65537, -2), (4, -1, -1), (4, 15, -1)):
        case.steps += [Call("lcp_link_jacobian_f64", with_size(k, v) + ins + fwd_tail, ("Je",), rc=rc),
                       Call("lcp_link_jacobian_backward_f64", with_size(k, v) + ins + grads, GRADS, rc=rc)]
    _run(case)
