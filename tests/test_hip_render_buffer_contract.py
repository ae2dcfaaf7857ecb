"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the drawing,
lcp_render_f64 and lcp_render_backward_f64: guard bands around every buffer, const inputs bitwise unchanged, each optional output
NULL in turn, vertex slots >= nverts never read, outputs written and not accumulated."""
import pytest
import torch

from tests import render_host as RH
from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = ("kind", "radius", "verts_local", "nverts", "p", "colors", "background", "thickness")
OUTS = ("image", "ids")
GRADS = ("g_p", "g_radius", "g_verts_local", "g_colors")


def _case(name, poison=None, twice=False, svm=None):
    """Case `name` of render_host.py with body 0 replaced by a rect that covers the image (so that every mask element is written
    with something other than the -1 the arena's fill reads as); `poison`: the value of the vertex slots >= nverts."""
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in RH.case(name).items()}
    B, nb, cap = c["verts_local"].shape[:3]
    H, W, C = c["H"], c["W"], c["colors"].shape[2]
    c["kind"][:, 0], c["nverts"][:, 0], c["thickness"][:, 0] = 1, 4, 0.0
    c["verts_local"][:, 0] = 0.0
    c["verts_local"][:, 0, :4] = torch.tensor(RH._rect(3000.0, 2000.0), dtype=F64)
    c["p"][:, 0] = torch.tensor([0.3, c["x0"] + 7.7, c["y0"] - 3.1], dtype=F64)
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    if poison is not None:
        c["verts_local"] = c["verts_local"].masked_fill(pad, poison)
    g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5), dtype=F32)
    bufs = [("kind", I32, (B, nb), "in", c["kind"]), ("radius", F64, (B, nb), "in", c["radius"]),
            ("verts_local", F64, (B, nb, cap, 2), "in", c["verts_local"]), ("nverts", I32, (B, nb), "in", c["nverts"]),
            ("p", F64, (B, nb, 3), "in", c["p"]), ("colors", F32, (B, nb, C), "in", c["colors"]), ("background", F32, (C,), "in", c["background"]),
            ("thickness", F64, (B, nb), "in", c["thickness"]), ("g_image", F32, (B, C, H, W), "in", g),
            ("image", F32, (B, C, H, W), "out", None), ("ids", I32, (B, H, W), "out", None),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_radius", F64, (B, nb), "out", None),
            ("g_verts_local", F64, (B, nb, cap, 2), "out", None), ("g_colors", F32, (B, nb, C), "out", None)]
    sizes = [B, nb, cap, int(nv.sum(1).max()) if svm is None else svm, H, W, C]
    cam = [c["x0"], c["y0"], c["ppm"], c["w"]]
    steps = [Call("lcp_render_f64", sizes + [R(n) for n in INS] + cam + [R(n) for n in OUTS], OUTS),
             Call("lcp_render_backward_f64", sizes + [R(n) for n in INS] + cam + [R("g_image")] + [R(n) for n in GRADS], GRADS)]

    def post(outs):
        assert int(outs["ids"].min()) >= 0 and int(outs["ids"].max()) < nb
        assert _absmax(outs["g_verts_local"][pad]) == 0.0, "slots >= nverts are not zero"
        assert _absmax(outs["g_radius"][hull]) == 0.0 and _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_colors"]) > 0.0

    # each optional output of either call NULL in turn, and the optional input
    nulls = [{n} for n in OUTS + GRADS]
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post), sizes, cam


@pytest.mark.parametrize("name,svm", [("three", None), ("special", None), ("nb33", None), ("nb64", None), ("three", 1024)])
def test_guards_optional_outputs_and_buffer_neighbourhood(name, svm):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn (19 x 23 is smaller than a tile, 40 x 70 no multiple of one; capacities
    8, 12 and 64; scene_verts_max = 1024: the largest LDS either kernel can ask for)."""
    _check(_case(name, svm=svm)[0])


@pytest.mark.parametrize("name", ["three", "special", "nb64"])
def test_slots_beyond_nverts_are_never_read(name):
    """Vertex slots >= nverts (all of a circle's) poisoned with NaN: every output finite and bit for bit what zeros there give."""
    clean = _check(_case(name)[0])
    dirty = _check(_case(name, poison=float("nan"))[0])
    for n in clean:
        assert _same(clean[n], dirty[n]), n


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers: the bits of one call."""
    once, _, _ = _run(_case("special")[0])
    twice, _, _ = _run(_case("special", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_a_null_thickness_is_every_body_filled():
    base, _, _ = _case("three")
    null, _, _ = _run(base, null=frozenset({"thickness"}))
    zero, _, _ = _case("three")
    zero.bufs = [(n, dt_, sh, role, torch.zeros(sh, dtype=dt_) if n == "thickness" else data) for n, dt_, sh, role, data in zero.bufs]
    want, _, _ = _run(zero)
    for n in OUTS + GRADS:
        assert _same(null[n], want[n]), n


def test_refusals_write_nothing():
    """A NULL required pointer, sizes outside the limits, a camera without scale: LCP_E_BADARG and no output touched."""
    case, sizes, cam = _case("three")
    ins = [R(n) for n in INS]
    outs, grads = [R(n) for n in OUTS], [R("g_image")] + [R(n) for n in GRADS]
    bad_in = ins[:4] + [R("p_missing")] + ins[5:]
    with_size = lambda k, v: sizes[:k] + [v] + sizes[k + 1:]
    case.steps = [Call("lcp_render_f64", sizes + bad_in + cam + outs, OUTS, rc=-1),
                  Call("lcp_render_backward_f64", sizes + bad_in + cam + grads, GRADS, rc=-1),
                  Call("lcp_render_backward_f64", sizes + ins + cam + [R("g_missing")] + grads[1:], GRADS, rc=-1)]
    for k, v in ((1, 65), (2, 7), (2, 65), (3, 1025), (4, 0), (5, 0), (6, 5), (6, 0)):
        case.steps += [Call("lcp_render_f64", with_size(k, v) + ins + cam + outs, OUTS, rc=-1),
                       Call("lcp_render_backward_f64", with_size(k, v) + ins + cam + grads, GRADS, rc=-1)]
    for bad_cam in (cam[:2] + [0.0, cam[3]], cam[:3] + [0.0], cam[:3] + [-1.0]):
        case.steps += [Call("lcp_render_f64", sizes + ins + bad_cam + outs, OUTS, rc=-1),
                       Call("lcp_render_backward_f64", sizes + ins + bad_cam + grads, GRADS, rc=-1)]
    _run(case)
