"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of lcp_contact_report_f32: guard bands around
every buffer, const inputs bitwise unchanged, every output fully written, each optional output NULL in turn, outputs written and not
accumulated, the same bits with the arena carved in reverse, refusals that write nothing."""
import pytest
import torch

from tests import contact_report_host as RH
from tests.test_hip_buffer_contract import E_TOOLARGE, F32, I32, Call, Case, R, _check, _run, _same

pytestmark = pytest.mark.gpu
RECORDS = ("c_n", "c_p1", "c_p2", "c_i1", "c_i2", "z")
INS = ("count", "active") + RECORDS + ("y", "Je", "first", "second")
FN = "lcp_contact_report_f32"


def _args(sizes, ins=None, outs=None, min_impulse=0.0):
    ins = [R(n) for n in INS] if ins is None else ins
    outs = [R(n) for n in RH.OUTPUTS] if outs is None else outs
    return list(sizes) + ins + [float(min_impulse)] + outs


def _case(name, twice=False):
    c, ref = RH.case(name), RH.reference(name)
    B, nb, maxc, e, P = RH.dims(c)
    shapes = {"count": (B,), "active": (B,), "c_n": (B, maxc, 2), "c_p1": (B, maxc, 2), "c_p2": (B, maxc, 2), "c_i1": (B, maxc),
              "c_i2": (B, maxc), "z": (B, 4 * maxc), "y": (B, e), "Je": (B, e, 3 * nb), "first": (B, P), "second": (B, P)}
    ints = ("count", "active", "c_i1", "c_i2", "first", "second")
    bufs = [(n, I32 if n in ints else F32, shapes[n], "in", c[n]) for n in INS if c[n] is not None]      # (an absent input: NULL)
    out_shapes = {"body_impulse": (B, nb, 3), "body_normal": (B, nb), "body_touching": (B, nb), "joint_impulse": (B, nb, 3),
                  "pair_impulse": (B, P, 3), "pair_normal": (B, P), "pair_contacts": (B, P)}
    bufs += [(n, I32 if n in RH.INTS else F32, out_shapes[n], "out", None) for n in RH.OUTPUTS]
    sizes = [B, nb, maxc, e, P]
    steps = [Call(FN, _args(sizes), RH.OUTPUTS)]

    def post(outs):
        for n in RH.OUTPUTS:
            if n in RH.INTS:
                assert torch.equal(outs[n], ref[n]), n
            else:
                assert RH.within_bound(outs[n], ref, n)[0], n
        assert float(outs["body_impulse"].abs().max()) > 0.0

    return Case(B, bufs, steps * (2 if twice else 1), nulls=[{n} for n in RH.OUTPUTS], post=post), sizes


@pytest.mark.parametrize("name", ["small", "edge65", "full"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn ("small": several scenes in one wavefront, a ragged last workgroup, no
    counts; "edge65": the first size on a group of 128 lanes; "full": the most bodies, records and pairs, the largest LDS)."""
    _check(_case(name)[0])


def test_outputs_are_overwritten_not_accumulated():
    """The call twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("small")[0])
    twice, _, _ = _run(_case("small", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """Sizes beyond the limits: LCP_E_TOOLARGE; a NULL record pointer, a NULL pair array with P > 0, a size below its lower limit or no
    output at all: LCP_E_BADARG; no output touched by any of them."""
    case, sizes = _case("small")
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    ins = [R(n) for n in INS]
    steps = [Call(FN, _args(with_size(1, 65)), RH.OUTPUTS, rc=E_TOOLARGE), Call(FN, _args(with_size(2, 1025)), RH.OUTPUTS, rc=E_TOOLARGE),
             Call(FN, _args(with_size(4, 1025)), RH.OUTPUTS, rc=E_TOOLARGE)]
    for k, v in ((0, -1), (1, 0), (2, 0), (3, -1), (4, -1)):
        steps.append(Call(FN, _args(with_size(k, v)), RH.OUTPUTS, rc=-1))
    for n in RECORDS + ("first", "second"):
        k = INS.index(n)
        steps.append(Call(FN, _args(sizes, ins=ins[:k] + [R("missing")] + ins[k + 1:]), RH.OUTPUTS, rc=-1))
    steps.append(Call(FN, _args(sizes, outs=[R("missing")] * 7), RH.OUTPUTS, rc=-1))
    case.steps = steps
    _run(case)
