"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the force
elements, lcp_force_elements_f64 and lcp_force_elements_backward_f64: guard bands around every buffer, const inputs bitwise unchanged,
every output fully written, each optional buffer NULL in turn, outputs written and not accumulated, the same bits with the arena carved
in reverse, refusals that write nothing."""
import pytest
import torch

from tests import force_elements_host as FH
from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = FH.ELEMENT_ARRAYS + ("p", "v")
GRADS = tuple("g_" + n for n in FH.LEAVES)
FAR = 1e30                       # stands for limit = inf in the arena (no tension of the cases comes near it)


def _case(name, twice=False):
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in FH.case(name).items()}
    c["limit"] = c["limit"].clamp(max=FAR)
    ref = FH.reference(name)
    assert float(ref["raw"].abs().max()) < 1e-3 * FAR
    B, nb = c["p"].shape[:2]
    E = c["kind"].shape[1]
    shape = lambda n: (B, E, 2) if n in ("a1", "a2") else (B, E)
    bufs = [(n, I32 if n in ("kind", "b1", "b2") else F64, shape(n), "in", c[n]) for n in FH.ELEMENT_ARRAYS]
    bufs += [("p", F64, (B, nb, 3), "in", c["p"]), ("v", F32, (B, nb, 3), "in", c["v"]), ("f_base", F32, (B, nb, 3), "in", c["f_base"]),
             ("g_f", F32, (B, nb, 3), "in", c["g_f"]), ("f_out", F32, (B, nb, 3), "out", None)]
    bufs += [("g_" + n, F64, (B, nb, 3) if n in ("p", "v") else shape(n), "out", None) for n in FH.LEAVES]
    sizes = [B, nb, E]
    steps = [Call("lcp_force_elements_f64", sizes + [R(n) for n in INS] + [R("f_base"), R("f_out")], ("f_out",)),
             Call("lcp_force_elements_backward_f64", sizes + [R(n) for n in INS] + [R("g_f")] + [R(n) for n in GRADS], GRADS)]

    def post(outs):
        bound = 2.0 ** -24 * ref["f64"].abs() + 1e-12 * ref["S"]
        assert bool(((outs["f_out"].double() - ref["f64"]).abs() <= bound).all())
        assert _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_k"] - ref["grads"]["k"]) <= 1e-8 * _absmax(ref["grads"]["k"])

    nulls = [{n} for n in GRADS]                                      # each optional gradient NULL in turn (f_base: its own test)
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post), sizes


@pytest.mark.parametrize("name", ["small", "edge65", "full"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional gradient NULL in turn ("small": several scenes in one wavefront; "edge65": the first size on a
    group of 128 lanes; "full": the most bodies and elements, the largest LDS either kernel asks for, two chunks in the backward)."""
    _check(_case(name)[0])


def test_a_missing_base_force_leaves_every_other_contract_in_place():
    """f_base NULL: guards intact, f_out fully written, and - with the case's f_base set to zero - the same bits as the given base."""
    case, _ = _case("small")
    zero = [(n, dt, sh, role, (torch.zeros(sh, dtype=dt) if n == "f_base" else data)) for n, dt, sh, role, data in case.bufs]
    with_zero, _, _ = _run(Case(case.B, zero, case.steps))
    without, _, _ = _run(case, null=frozenset({"f_base"}))
    assert bool(torch.isfinite(without["f_out"]).all()) and _same(with_zero["f_out"], without["f_out"])


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("small")[0])
    twice, _, _ = _run(_case("small", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """A NULL required pointer, sizes outside the limits, no output: LCP_E_BADARG and no output touched."""
    case, sizes = _case("small")
    ins = [R(n) for n in INS]
    fwd_tail, grads = [R("f_base"), R("f_out")], [R("g_f")] + [R(n) for n in GRADS]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    case.steps = [Call("lcp_force_elements_backward_f64", sizes + ins + [R("g_missing")] + grads[1:], GRADS, rc=-1),
                  Call("lcp_force_elements_backward_f64", sizes + ins + [R("g_f")] + [R("missing")] * 8, GRADS, rc=-1),
                  Call("lcp_force_elements_f64", sizes + ins + [R("f_base"), R("missing")], ("f_out",), rc=-1)]
    for k in range(len(INS)):
        bad_in = ins[:k] + [R("missing")] + ins[k + 1:]
        case.steps += [Call("lcp_force_elements_f64", sizes + bad_in + fwd_tail, ("f_out",), rc=-1),
                       Call("lcp_force_elements_backward_f64", sizes + bad_in + grads, GRADS, rc=-1)]
    for k, v in ((0, -1), (1, 0), (1, 65), (2, 0), (2, 1025)):
        case.steps += [Call("lcp_force_elements_f64", with_size(k, v) + ins + fwd_tail, ("f_out",), rc=-1),
                       Call("lcp_force_elements_backward_f64", with_size(k, v) + ins + grads, GRADS, rc=-1)]
    _run(case)
