"""GPU: the buffer contract (tests/test_hip_buffer_contract.py, on tests/guarded_buffers.py) of the two entry points of the drawing
with marks and joint markers, lcp_render_marks_f64 and lcp_render_marks_backward_f64: guard bands around every buffer, const inputs
bitwise unchanged, each optional output NULL in turn, outputs written and not accumulated, the refusals before any launch."""
import pytest
import torch

from tests import render_host as RH
from tests import render_marks_host as MH
from tests.test_hip_buffer_contract import F32, F64, I32, Call, Case, R, _absmax, _check, _run, _same

pytestmark = pytest.mark.gpu
INS = ("kind", "radius", "verts_local", "nverts", "p", "colors", "background", "thickness")
MARKS = ("mark", "mark_colors")
JOINTS = ("jtype", "jb1", "jb2", "jr1", "jrot1", "joint_colors")
OUTS = ("image", "ids")
GRADS = ("g_p", "g_radius", "g_verts_local", "g_colors", "g_mark_colors", "g_joint_colors", "g_jrot1", "g_jr1")
WS = "g_p_joints"


def _case(name, twice=False):
    """Case `name` of render_marks_host.py with body 0 replaced by a rect that covers the image (so that every mask element is written
    with something other than the -1 the arena's fill reads as).  A case without joints carves no joint buffer: NULL pointers."""
    c = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in MH.case(name).items()}
    B, nb, cap = c["verts_local"].shape[:3]
    H, W, C = c["H"], c["W"], c["colors"].shape[2]
    nj = c["jtype"].shape[1]
    c["kind"][:, 0], c["nverts"][:, 0], c["thickness"][:, 0] = 1, 4, 2.5
    c["verts_local"][:, 0] = 0.0
    c["verts_local"][:, 0, :4] = torch.tensor(RH._rect(3000.0, 2000.0), dtype=F64)
    c["p"][:, 0] = torch.tensor([0.3, c["x0"] + 7.7, c["y0"] - 3.1], dtype=F64)
    c["mark"][:, 0] = MH.DIAGONALS
    hull = c["kind"] != 0
    nv = c["nverts"] * hull
    pad = (torch.arange(cap).reshape(1, 1, cap) >= nv.unsqueeze(2)).unsqueeze(3).expand(B, nb, cap, 2)
    g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5), dtype=F32)
    bufs = [("kind", I32, (B, nb), "in", c["kind"]), ("radius", F64, (B, nb), "in", c["radius"]),
            ("verts_local", F64, (B, nb, cap, 2), "in", c["verts_local"]), ("nverts", I32, (B, nb), "in", c["nverts"]),
            ("p", F64, (B, nb, 3), "in", c["p"]), ("colors", F32, (B, nb, C), "in", c["colors"]), ("background", F32, (C,), "in", c["background"]),
            ("thickness", F64, (B, nb), "in", c["thickness"]), ("mark", I32, (B, nb), "in", c["mark"]),
            ("mark_colors", F32, (B, nb, C), "in", c["mark_colors"]), ("g_image", F32, (B, C, H, W), "in", g),
            ("image", F32, (B, C, H, W), "out", None), ("ids", I32, (B, H, W), "out", None),
            ("g_p", F64, (B, nb, 3), "out", None), ("g_radius", F64, (B, nb), "out", None),
            ("g_verts_local", F64, (B, nb, cap, 2), "out", None), ("g_colors", F32, (B, nb, C), "out", None),
            ("g_mark_colors", F32, (B, nb, C), "out", None)]
    if nj:
        bufs += [("jtype", I32, (B, nj), "in", c["jtype"]), ("jb1", I32, (B, nj), "in", c["jb1"]), ("jb2", I32, (B, nj), "in", c["jb2"]),
                 ("jr1", F64, (B, nj), "in", c["jr1"]), ("jrot1", F64, (B, nj), "in", c["jrot1"]),
                 ("joint_colors", F32, (B, nj, C), "in", c["joint_colors"]),
                 ("g_joint_colors", F32, (B, nj, C), "out", None), ("g_jrot1", F64, (B, nj), "out", None), ("g_jr1", F64, (B, nj), "out", None),
                 (WS, F64, (B, nj, 2, 3), "out", None)]
    sizes = [B, nb, cap, int(nv.sum(1).max()), H, W, C]
    cam = [c["x0"], c["y0"], c["ppm"], c["w"]]
    tail = [c["order"], c["line_w"], c["dot_r"], c["joint_w"], c["joint_r"]]
    head = sizes + [R(n) for n in INS] + cam + [R(n) for n in MARKS] + [nj] + [R(n) for n in JOINTS] + tail
    steps = [Call("lcp_render_marks_f64", head + [R(n) for n in OUTS], OUTS),
             Call("lcp_render_marks_backward_f64", head + [R("g_image")] + [R(n) for n in GRADS] + [R(WS)], GRADS + (WS,))]

    def post(outs):
        assert int(outs["ids"].min()) >= 0 and int(outs["ids"].max()) < nb
        assert _absmax(outs["g_verts_local"][pad]) == 0.0, "slots >= nverts are not zero"
        assert _absmax(outs["g_radius"][hull]) == 0.0 and _absmax(outs["g_p"]) > 0.0 and _absmax(outs["g_colors"]) > 0.0
        assert _absmax(outs["g_mark_colors"]) > 0.0
        if nj:
            assert _absmax(outs["g_joint_colors"]) > 0.0 and _absmax(outs["g_jrot1"]) > 0.0 and _absmax(outs["g_jr1"]) > 0.0
            assert _absmax(outs["g_jrot1"][c["jtype"] != MH.JOINT]) == 0.0 and _absmax(outs["g_jr1"][c["jtype"] != MH.JOINT]) == 0.0
            assert _absmax(outs[WS][..., 0]) == 0.0 and _absmax(outs[WS]) > 0.0

    # each optional output of either call NULL in turn; the workspace only together with the pose gradient that needs it
    names = [n for n in OUTS + GRADS if nj or n not in ("g_joint_colors", "g_jrot1", "g_jr1")]
    nulls = [{n} for n in names] + ([{"g_p", WS}] if nj else []) + [{"mark", "mark_colors", "g_mark_colors"}]
    nulls = [s for s in nulls if "mark" not in s]                    # (without marks the image itself differs: its own test)
    return Case(B, bufs, steps * (2 if twice else 1), nulls=nulls, post=post), head, nj


@pytest.mark.parametrize("name", ["marks3", "marks3_over", "joints", "limits"])
def test_guards_optional_outputs_and_buffer_neighbourhood(name):
    """Guards intact, inputs const, every promised element written and finite, the same bits with the arena carved in reverse and
    zero-filled, and with each optional output NULL in turn (19 x 23 is smaller than a tile, 40 x 70 no multiple of one; 64 bodies
    and 64 joints: every table full)."""
    _check(_case(name)[0])


def test_outputs_are_overwritten_not_accumulated():
    """Both calls twice into the same buffers (the workspace and the second launch's sum into g_p included): the bits of one call."""
    once, _, _ = _run(_case("joints")[0])
    twice, _, _ = _run(_case("joints", twice=True)[0])
    for n in once:
        assert _same(once[n], twice[n]), n


def test_refusals_write_nothing():
    """LCP_E_BADARG before any launch and no output touched: nj outside 0..64, an order other than 0 / 1, a width that is not
    positive, a negative radius, a NULL required pointer, g_p asked for with joints and no workspace, no output requested."""
    case, head, nj = _case("joints")
    outs, grads = [R(n) for n in OUTS], [R("g_image")] + [R(n) for n in GRADS] + [R(WS)]
    i_nj, i_order = 7 + 8 + 4 + 2, 7 + 8 + 4 + 2 + 1 + 6
    at = lambda k, v: head[:k] + [v] + head[k + 1:]
    bad_heads = [at(i_nj, -1), at(i_nj, 65), at(i_order, 2), at(i_order, -1),
                 at(i_order + 1, 0.0), at(i_order + 1, -1.0), at(i_order + 3, 0.0), at(i_order + 3, float("nan")),      # line_w, joint_w
                 at(i_order + 2, -1e-9), at(i_order + 4, -1.0),                                                       # dot_r, joint_r
                 at(7 + 4, R("p_missing")), at(7 + 8 + 4 + 1, R("mark_colors_missing")),                               # p, mark_colors
                 at(i_nj + 1, R("jtype_missing")), at(i_nj + 5, R("jrot1_missing")), at(i_nj + 6, R("joint_colors_missing"))]
    case.steps = []
    for h in bad_heads:
        case.steps += [Call("lcp_render_marks_f64", h + outs, OUTS, rc=-1),
                       Call("lcp_render_marks_backward_f64", h + grads, GRADS + (WS,), rc=-1)]
    case.steps += [Call("lcp_render_marks_backward_f64", head + grads[:-1] + [R("workspace_missing")], GRADS + (WS,), rc=-1),
                   Call("lcp_render_marks_backward_f64", head + [R("g_missing")] + grads[1:], GRADS + (WS,), rc=-1),
                   Call("lcp_render_marks_f64", head + [R("none"), R("none")], OUTS, rc=-1),
                   Call("lcp_render_marks_backward_f64", head + [R("g_image")] + [R("none")] * 8 + [R(WS)], GRADS + (WS,), rc=-1)]
    _run(case)
